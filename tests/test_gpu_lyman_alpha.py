"""GPU tests of the Lyman-alpha transfer (include/cmi_gpu.h, "Lyman alpha";
DESIGN.md 4.17): cmi_gpu_set_lyman_alpha, cmi_gpu_lya_shoot, the probes, the
downloads and GpuEngine.render_lyman_alpha_cube - against the CPU restatement
tests/support/lyman_alpha_reference.c on the same random streams (checked on
its own in test_lyman_alpha_host.py) and against the identities of the
contract.

Scene: lyman_alpha_lib.parity_scene, a 12^3 box with a density bump, a
temperature gradient, an expanding velocity field and dust; a packet scatters
some 250 times. The odd grid 6 x 5 x 7 serves the probes.

Tolerances. eps = 2^-52. The device's and glibc's exp, log, sin, cos, tan,
atan and pow are each within 1 ulp of the exact value, hence within 2 ulp of
each other; everything else is the same IEEE operation on both sides.
  H = sqrt(pi) Q + exp(-x^2): Q is the same bits, the exp differs by 2 ulp,
  the sum rounds once more: |dH| <= 4 eps H; kappa = kappa_0 H + kappa_d two
  more roundings that are the same on both sides given H: <= 6 eps kappa.
  An optical depth is a sum of n <= 64 terms ds kappa of one sign, each off by
  at most 6 eps of itself, summed in the same order: <= (6 + 2) eps tau for
  the terms plus nothing for the order; held to 16 eps tau.
  u_par = a tan(th) + |x| with th = c + R (th_0 - c): th_0 = atan(..) is off
  by 2 ulp of a number below pi / 2, th by that and its own rounding (4 eps
  pi / 2), tan(th) by sec^2(th) times that and 2 ulp of itself:
  |du| <= a (1 + t^2) 8 eps + 4 eps |a t| + 2 eps |u|, t = (u - |x|) / a.
  Traces. A resonant scattering carries an error dx of the frequency on as mu
  dx (mu the cosine of the scattering angle: the atom's u_par follows x), so
  the walk does not amplify rounding; the scatterings off the fast atoms of
  the core multiply it by up to |1 + 1.2 (u - x)(mu - 1)| < 20 and are a few
  per cent of all. Over the 48 events of a row the columns are held to: q
  and u within 1e-9 b, positions within 1e-9 of a cell side, x within 1e-9,
  u_par by the bound above plus 1e-9; an addend, exp(-tau) of a depth of up to
  a few hundred whose relative error is 2 x dx per unit depth, within 1e-6 of
  itself plus 1e-12 of the largest. The measured worst cases are printed (and
  stand in DESIGN.md 4.17): they are orders of magnitude inside.
  Whole runs. An element of the image or of the cube is a sum of addends, each
  within 1e-6 of itself as above but with the bulk of the light in addends of
  small depth (relative error 1e-9 and below): an element is held to 1e-8 of
  its pixel's image value, and elements beyond that are traced to their
  packets by bisection, as test_gpu_scattered_cube.py does, and those must be
  threshold cases: a decision of the restatement within 1e-9 of its threshold,
  an event within 1e-9 cell sides of a wall, within 1e-9 of a channel edge or
  on a pixel edge (the trace's pixel differs). At most 1 % of the packets may
  be excused this way."""
import numpy as np
import pytest

import lyman_alpha_lib as Y
import scattered_cube_lib as Q

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
SEED = 7
N = 20000


@pytest.fixture(scope="module")
def parity():
    scene, box = Y.parity_scene()
    eng = scene.engine()
    yield scene, eng
    eng.close()


@pytest.fixture(scope="module")
def small():
    """the odd grid of the probes: 6 x 5 x 7"""
    scene, box = Y.parity_scene(ncell=(6, 5, 7), nx=7, ny=5, sigma_turb=2.0e3)
    eng = scene.engine()
    yield scene, eng
    eng.close()


def _run(eng, seed, first, n):
    eng.reset_lya()
    eng.lya_shoot(seed, first, n)
    image, cube = eng.download_lya()
    return image[0], cube[0], eng.get_lya_counters()


# ------------------------------------------------------------- probes --

def test_voigt_and_opacity_rows(small):
    scene, eng = small
    ref = Y.Restatement(scene)
    rng = np.random.default_rng(3)
    x = np.r_[0., np.sqrt(0.855), 7.999, 8., 8.001, -2.5, 1000.,
              rng.normal(0., 3., 4000), 10. ** rng.uniform(0., 3., 1000)]
    a = 10. ** rng.uniform(-4., -1.7, len(x))
    rows = np.stack([a, x, 10. ** rng.uniform(-18., -12., len(x)),
                     10. ** rng.uniform(-20., -14., len(x))], axis=1)
    gpu = eng.lya_probe(Y.VOIGT, rows=rows)
    cpu = ref.voigt(rows)
    dH = np.abs(gpu[:, 0] - cpu[:, 0]) / cpu[:, 0]
    dk = np.abs(gpu[:, 1] - cpu[:, 1]) / cpu[:, 1]
    print("worst dH / eps", dH.max() / EPS, "dkappa / eps", dk.max() / EPS)
    assert dH.max() <= 4. * EPS and dk.max() <= 6. * EPS
    # beyond the cut both sides leave the exp out: the same bits
    far = x * x >= 64.
    assert far.sum() > 100 and np.array_equal(gpu[far], cpu[far])


def test_optical_depth_rows(small):
    scene, eng = small
    ref = Y.Restatement(scene)
    m = scene.m
    rng = np.random.default_rng(4)
    n = 3000
    pos = m.anchor + rng.uniform(0., 1., (n, 3)) * m.sides
    d = rng.normal(size=(n, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    d[:6] = np.r_[np.eye(3), -np.eye(3)]  # along the axes: 1 / 0 components
    q = rng.normal(0., 4.0e4, n)
    rows = np.c_[pos, d, q]
    gpu = eng.lya_probe(Y.OPTICAL_DEPTH, rows=rows)
    cpu = ref.optical_depth(rows)
    assert np.array_equal(gpu[:, 1], cpu[:, 1]) and cpu[:, 1].max() <= 64
    err = np.abs(gpu[:, 0] - cpu[:, 0]) / cpu[:, 0]
    print("worst dtau / (eps tau)", err.max() / EPS, "tau", cpu[:, 0].min(),
          cpu[:, 0].max())
    assert err.max() <= 16. * EPS
    assert cpu[:, 0].max() > 1.0e3 * cpu[:, 0].min() > 0.


def test_atom_sampler_rows(small):
    scene, eng = small
    ref = Y.Restatement(scene)
    rng = np.random.default_rng(5)
    n = 20000
    x = np.r_[rng.normal(0., 2.5, n - 2000), rng.uniform(-12., 12., 1900),
              rng.uniform(-1000., 1000., 100)]
    a = 10. ** rng.uniform(-3.9, -1.8, n)
    rows = np.c_[x, a]
    gpu = eng.lya_probe(Y.SAMPLER, seed=SEED, first_packet=100, rows=rows)
    cpu, margins = ref.sampler(SEED, 100, rows)
    keep = margins > 1e-9
    print("left out", int((~keep).sum()), "of", n)
    assert (~keep).sum() <= 0.01 * n
    assert np.array_equal(gpu[keep, 1], cpu[keep, 1])
    u = cpu[keep, 0]
    t = (np.abs(u) - np.abs(x[keep])) / a[keep]
    tol = a[keep] * (1. + t * t) * 8. * EPS + 4. * EPS * np.abs(a[keep] * t) \
        + 2. * EPS * np.abs(u)
    err = np.abs(gpu[keep, 0] - u)
    print("worst du / tol", (err / tol).max(), "rejections per draw",
          cpu[:, 1].mean())
    assert np.all(err <= tol)
    assert np.array_equal(np.sign(gpu[keep, 0]) , np.sign(u))


def test_probe_rows_past_one_launch(small):
    """More rows than one launch of cmi_gpu_lya_probe takes (2^14): the rows
    past it are the rows probed alone, with first_packet moved up by 2^14."""
    scene, eng = small
    rng = np.random.default_rng(6)
    launch = 1 << 14
    n = launch + 50
    rows = np.c_[rng.normal(0., 2.5, n), 10. ** rng.uniform(-3.9, -1.8, n)]
    gpu = eng.lya_probe(Y.SAMPLER, seed=SEED, first_packet=100, rows=rows)
    alone = eng.lya_probe(Y.SAMPLER, seed=SEED, first_packet=100 + launch,
                          rows=rows[launch:])
    assert np.abs(gpu[launch:, 0]).min() > 0.
    assert np.array_equal(gpu[launch:], alone)


def test_traces(parity):
    """the first TRACE_EVENTS events of TRACE_PACKETS packets, row by row; no
    row is left out (test_lyman_alpha_host.py::test_parity_seeds_need_no_
    excuse)"""
    scene, eng = parity
    ref = Y.Restatement(scene)
    n, cap = Y.TRACE_PACKETS, Y.TRACE_EVENTS
    gpu = eng.lya_probe(Y.TRACE, seed=Y.TRACE_SEED, n=n, max_events=cap)
    cpu, margins = ref.trace(Y.TRACE_SEED, 0, n, cap)
    assert margins.min() > 1e-9
    assert np.array_equal(gpu[:, :6], cpu[:, :6])
    assert np.all(gpu[:, 4] == 0.)
    g = gpu[:, Y.HEADER:].reshape(n, cap, Y.ROW)
    c = cpu[:, Y.HEADER:].reshape(n, cap, Y.ROW)
    have = np.arange(cap)[None, :] < np.minimum(cpu[:, 0], cap)[:, None]
    g, c = g[have], c[have]
    assert len(c) > 5000
    assert np.array_equal(g[:, 8], c[:, 8])
    assert (c[:, 8] == 1.).sum() > 1000 and (c[:, 8] == 2.).sum() > 10
    b = Y.doppler_width(scene.T).min()
    side = (scene.m.sides / scene.m.ncell).min()
    worst = {
        "pos / side": np.abs(g[:, 0:3] - c[:, 0:3]).max() / side,
        "k": np.abs(g[:, 3:6] - c[:, 3:6]).max(),
        "q / b": np.abs(g[:, 6] - c[:, 6]).max() / b,
        "u / b": np.abs(g[:, 9] - c[:, 9]).max() / b,
        "x": np.abs(g[:, 11] - c[:, 11]).max(),
        "u_par": np.abs(g[:, 10] - c[:, 10]).max(),
        "addend": (np.abs(g[:, 7] - c[:, 7]) /
                   (1e-6 * np.abs(c[:, 7]) + 1e-12 * c[:, 7].max())).max()}
    print("worst", worst)
    assert worst["pos / side"] <= 1e-9 and worst["k"] <= 1e-9
    assert worst["q / b"] <= 1e-9 and worst["u / b"] <= 1e-9
    assert worst["x"] <= 1e-9 and worst["addend"] <= 1.
    hyd = c[:, 8] == 1.
    a = Y.voigt_parameter(b)
    t = (np.abs(c[hyd, 10]) - np.abs(c[hyd, 11])) / a
    tol = a * (1. + t * t) * 8. * EPS + 4. * EPS * np.abs(a * t) + \
        2. * EPS * np.abs(c[hyd, 10]) + 1e-9
    assert np.all(np.abs(g[hyd, 10] - c[hyd, 10]) <= tol)
    # the rows are not constants of the scene
    assert np.ptp(c[:, 9]) > 1.0e5 and np.ptp(c[hyd, 10]) > 4.


def test_a_packet_alone_is_the_packet_among_others(parity):
    scene, eng = parity
    cap = 16
    among = eng.lya_probe(Y.TRACE, seed=SEED, n=64, max_events=cap)
    for k in (0, 1, 31, 32, 63, int(np.argmax(among[:, 1]))):
        alone = eng.lya_probe(Y.TRACE, seed=SEED, first_packet=k, n=1,
                              max_events=cap)[0]
        assert np.array_equal(alone, among[k]), k


# --------------------------------------------------------- whole runs --

def _bad(gpu, cpu, image):
    return np.abs(gpu - cpu) > 1e-8 * image


def _culprits(eng, ref, lo, hi, out):
    image, cube, _ = _run(eng, SEED, lo, hi - lo)
    cimage, ccube, _, _ = ref.shoot(SEED, lo, hi - lo)
    if not (_bad(cube, ccube, cimage[None]).any() or
            _bad(image, cimage, cimage).any()):
        return
    if hi - lo == 1:
        out.append(lo)
        return
    mid = (lo + hi) // 2
    _culprits(eng, ref, lo, mid, out)
    _culprits(eng, ref, mid, hi, out)


def _is_threshold_case(scene, eng, ref, k):
    cap = 4096
    ct, margin = ref.trace(SEED, k, 1, cap)
    if margin[0] <= 1e-9:
        return True
    rows, _ = Y.events(ct, cap)
    if Q.near_wall(scene.m, rows[:, 0:3]).any():
        return True
    f = (rows[:, 9] - scene.vmin) / ((scene.vmax - scene.vmin) / scene.nchan)
    if np.abs(f - np.round(f)).min() <= 1e-9:
        return True
    # an event on a pixel edge: the pixel of the traced position differs
    # between the positions of the two sides
    gt = eng.lya_probe(Y.TRACE, seed=SEED, first_packet=k, n=1,
                       max_events=cap)
    grows, _ = Y.events(gt, cap)
    if len(grows) != len(rows):
        return True
    return any(ref.pixel(a) != ref.pixel(b)
               for a, b in zip(grows[:, 0:3], rows[:, 0:3]))


def test_whole_run(parity):
    """2e4 packets, image and cube per element (the module docstring has the
    bound and the excuse)"""
    scene, eng = parity
    ref = Y.Restatement(scene)
    image, cube, c = _run(eng, SEED, 0, N)
    cimage, ccube, cc, _ = ref.shoot(SEED, 0, N)
    assert c["npackets"] == N and c["ncapped"] == 0 and cc["ncapped"] == 0
    assert cc["nhydrogen"] > 50 * N and cc["ndust"] > N / 10
    assert np.count_nonzero(ccube) > 500
    bad = _bad(cube, ccube, cimage[None])
    worst = (np.abs(cube - ccube) / (cimage[None] + 1e-300)).max()
    print("differing elements", int(bad.sum()), "worst", worst,
          "image worst", (np.abs(image - cimage) / (cimage + 1e-300)).max())
    culprits = []
    if bad.any() or _bad(image, cimage, cimage).any():
        _culprits(eng, ref, 0, N, culprits)
        print("culprits", culprits)
        assert 0 < len(culprits) <= 0.01 * N
        for k in culprits:
            assert _is_threshold_case(scene, eng, ref, k), k
        # the run without them agrees
        for k in culprits:
            gi, gc, _ = _run(eng, SEED, k, 1)
            ci, ccu, _, _ = ref.shoot(SEED, k, 1)
            image, cube = image - gi, cube - gc
            cimage, ccube = cimage - ci, ccube - ccu
        assert not _bad(cube, ccube, np.abs(cimage)[None] + 1e-9 *
                        cimage.max()).any()
    else:
        for name in ("nsteps", "nhydrogen", "ndust", "nrejections",
                     "natomics", "npackets"):
            assert c[name] == cc[name], name


@pytest.mark.parametrize("n", [3, 67])
def test_partial_wave(parity, n):
    scene, eng = parity
    ref = Y.Restatement(scene)
    image, cube, c = _run(eng, SEED, 1000, n)
    cimage, ccube, cc, margin = ref.shoot(SEED, 1000, n)
    assert margin > 1e-9
    assert c["npackets"] == n == cc["npackets"]
    assert c["nhydrogen"] == cc["nhydrogen"] and c["nsteps"] == cc["nsteps"]
    assert not _bad(cube, ccube, cimage[None]).any()
    assert not _bad(image, cimage, cimage).any()


def test_additive(parity):
    """[0, N / 2) + [N / 2, N) against [0, N): the order of the atomics only"""
    scene, eng = parity
    n = 4000
    whole = _run(eng, SEED, 0, n)
    eng.reset_lya()
    eng.lya_shoot(SEED, 0, n // 2)
    eng.lya_shoot(SEED, n // 2, n - n // 2)
    image, cube = eng.download_lya()
    c = eng.get_lya_counters()
    assert c == whole[2]
    assert np.allclose(image[0], whole[0], rtol=1e-12, atol=0.)
    assert np.allclose(cube[0], whole[1], rtol=1e-12,
                       atol=1e-14 * whole[0].max())


def test_three_views_against_three_single_cameras():
    views = [(1.1, 0.6), (0.3, 2.0), (np.pi / 2., 0.)]
    n = 2000
    scene, _ = Y.parity_scene()
    eng = scene.engine(views)
    eng.lya_shoot(SEED, 0, n)
    images, cubes = eng.download_lya()
    counters = eng.get_lya_counters()
    eng.close()
    assert images.shape == (3, 12, 12) and cubes.shape == (3, 16, 12, 12)
    steps = 0
    for v, (theta, phi) in enumerate(views):
        one, _ = Y.parity_scene(view=(theta, phi))
        one.m.img_anchor, one.m.img_sides = scene.m.img_anchor, \
            scene.m.img_sides
        e1 = one.engine()
        image, cube, c = _run(e1, SEED, 0, n)
        e1.close()
        assert image.sum() > 0.
        assert np.allclose(images[v], image, rtol=1e-12, atol=0.), v
        assert np.allclose(cubes[v], cube, rtol=1e-12,
                           atol=1e-14 * image.max()), v
        assert c["nhydrogen"] == counters["nhydrogen"]
        steps += c["nsteps"]
    # the walk is shared, the peel-off marches are per view
    assert counters["nsteps"] < steps


def test_three_views_past_the_first_launch():
    """The several-views instantiation through the chunk loop of
    cmi_gpu_lya_shoot past its first launch of 2^14 packets (test_whole_run
    crosses it with one view): [0, n) in one call against [0, 2^14) and
    [2^14, n) in two, on an 8^3 grid with 16 x 16 images. The counters are
    equal, images and cubes differ by the order of the atomics."""
    views = [(1.1, 0.6), (0.3, 2.0), (np.pi / 2., 0.)]
    first = 1 << 14
    n = first + 100
    scene, _ = Y.parity_scene(ncell=(8, 8, 8), nx=16, ny=16, tau0=30.)
    eng = scene.engine(views)
    eng.lya_shoot(SEED, 0, n)
    images, cubes = eng.download_lya()
    c = eng.get_lya_counters()
    eng.reset_lya()
    eng.lya_shoot(SEED, 0, first)
    eng.lya_shoot(SEED, first, n - first)
    images2, cubes2 = eng.download_lya()
    c2 = eng.get_lya_counters()
    eng.close()
    assert c["npackets"] == n and c["ncapped"] == 0 and c["nhydrogen"] > n
    assert c2 == c
    for v in range(3):
        assert images[v].sum() > 0.
        atol = 1e-14 * images[v].max()
        assert np.allclose(images2[v], images[v], rtol=1e-12, atol=atol), v
        assert np.allclose(cubes2[v], cubes[v], rtol=1e-12, atol=atol), v


# --------------------------------------------------------- identities --

def test_identities(parity):
    """one covering channel is the image; covering channels sum to it; a
    Galilean shift by three channels (the restatement's own tests have the
    reasons)"""
    scene, eng = parity
    n = 3000
    try:
        eng.set_lyman_alpha(1, -1.0e7, 1.0e7, 0., 0., Y.MAX_SCATTER,
                            scene.n_HI, scene.T)
        image, cube, _ = _run(eng, SEED, 0, n)
        assert np.allclose(cube[0], image, rtol=1e-12, atol=0.)
        eng.set_lyman_alpha(5, -1.0e7, 1.0e7, 0., 0., Y.MAX_SCATTER,
                            scene.n_HI, scene.T)
        image5, cube5, _ = _run(eng, SEED, 0, n)
        assert np.allclose(image5, image, rtol=1e-12, atol=0.)
        assert np.allclose(cube5.sum(axis=0), image, rtol=1e-12, atol=0.)
        m = scene.m
        d = np.array([np.sin(m.theta) * np.cos(m.phi),
                      np.sin(m.theta) * np.sin(m.phi), np.cos(m.theta)])
        nchan, vmin, vmax = 20, -2.0e5, 2.0e5
        dv = (vmax - vmin) / nchan
        V = 3. * dv * d + 1.7e4 * np.cross(d, [0., 0., 1.])
        eng.set_lyman_alpha(nchan, vmin, vmax, 0., 0., Y.MAX_SCATTER,
                            scene.n_HI, scene.T)
        _, cube, _ = _run(eng, SEED, 0, n)
        eng.set_cell_velocities(Y._f64(scene.velocity + V[:, None]))
        eng.set_lyman_alpha(nchan, vmin, vmax, 0., 0., Y.MAX_SCATTER,
                            scene.n_HI, scene.T)
        _, moved, _ = _run(eng, SEED, 0, n)
        assert np.allclose(moved[:-3], cube[3:], rtol=1e-9,
                           atol=1e-12 * cube.max())
        assert cube[3:].sum() > 0.9 * cube.sum()
    finally:
        scene.apply(eng)


def test_without_hydrogen_and_dust_it_is_the_thin_gaussian_line():
    """the restatement's test on the device, through
    render_lyman_alpha_cube's scaling: per pixel and channel against the
    restatement (the same packets: elementwise) and so against the ray-traced
    cube"""
    scene, box = Y.parity_scene(nchan=8, vmin=-3.2e4, vmax=3.2e4, nx=10,
                                ny=10, dust=False)
    scene.n_HI[:] = 0.
    ref = Y.Restatement(scene)
    n = 50000
    eng = scene.engine()
    image, cube, c = _run(eng, 11, 0, n)
    eng.close()
    cimage, ccube, cc, _ = ref.shoot(11, 0, n)
    assert c["nhydrogen"] == 0 and c["ndust"] == 0 and c["nsteps"] == \
        cc["nsteps"]
    assert np.allclose(image, cimage, rtol=1e-12, atol=0.)
    # an event within rounding of a channel edge may change channel
    off = np.abs(cube - ccube) > 1e-12 * cimage[None]
    print("elements off", int(off.sum()))
    assert off.sum() <= 2


# ------------------------------------------------------ static sphere --

def test_static_sphere():
    scene, b, a = Y.sphere_scene()
    eng = scene.engine()
    n = Y.SPHERE_PACKETS
    image, cube, c = _run(eng, Y.SPHERE_SEED, 0, n)
    eng.close()
    expected = Y.static_sphere_median(Y.SPHERE_A_TAU0)
    median, blue = Y.sphere_statistics(cube, scene, b)
    print("median |x|", median, "expected", expected, "blue share", blue,
          "scatterings per packet", c["nhydrogen"] / n)
    assert c["ncapped"] == 0 and c["ndust"] == 0 and c["npackets"] == n
    assert cube.sum() > 0.999 * image.sum()
    assert abs(median / expected - 1.) <= 0.05
    assert abs(blue - 0.5) <= 4. * np.sqrt(0.25 / n)


# ------------------------------------------- the Python entry points --

def test_render_lyman_alpha_cube_and_emissivity():
    """the scaling of render_lyman_alpha_cube, its views, and the emissivity
    of the cells against the formula in numpy"""
    from cmacionize_amd import engine as E
    scene, box = Y.parity_scene()
    m = scene.m
    eng = E.GpuEngine(tuple(int(v) for v in m.ncell), tuple(m.anchor),
                      tuple(m.sides), (0, 0, 0), device=0)
    x = np.zeros((E.NION, m.n))
    x[0] = 1.0e-4 * (1. + np.arange(m.n) % 7)
    x[1] = 0.3
    eng.upload_cells(m.density, scene.T, x)
    A_He = 0.08
    eng.set_abundances([A_He, 2.2e-4, 4.0e-5, 3.3e-4, 5.0e-5, 9.0e-6])
    j = eng.lyman_alpha_emissivity()
    T = scene.T
    Lm = 315614. / T
    alpha_B = 2.753e-14 * Lm ** 1.5 / (1. + (Lm / 2.74) ** 0.407) ** 2.242 \
        * 1e-6
    f_alpha = 0.686 - 0.106 * np.log10(T / 1e4) - 0.009 * (T / 1e4) ** -0.44
    n_e = m.density * ((1. - x[0]) + A_He * (1. - x[1]))
    expect = f_alpha * alpha_B * n_e * m.density * (1. - x[0]) * \
        (E.PLANCK * E.LIGHTSPEED / Y.LAMBDA0)
    assert np.allclose(j, expect, rtol=1e-12, atol=0.)
    n = 2000
    args = (m.nx, m.ny, m.img_anchor, m.img_sides, n, SEED, scene.nchan,
            scene.vmin, scene.vmax)
    image, cube = eng.render_lyman_alpha_cube(m.theta, m.phi, *args)
    assert image.shape == (m.nx, m.ny) and cube.shape == (scene.nchan, m.nx,
                                                          m.ny)
    assert image.sum() > 0. and np.all(cube.sum(axis=0) <= image * (1 + 1e-12))
    centres = E.cube_channel_centres(scene.nchan, scene.vmin, scene.vmax)
    m0, mean, sigma = E.cube_moments(cube, centres)
    assert np.allclose(m0, cube.sum(axis=0))
    images, cubes = eng.render_lyman_alpha_cube([m.theta, 0.3], [m.phi, 2.],
                                                *args)
    assert np.allclose(images[0], image, rtol=1e-12, atol=0.)
    assert np.allclose(cubes[0], cube, rtol=1e-12, atol=1e-14 * image.max())
    # the mode is left off
    with pytest.raises(E.EngineError, match="not set"):
        eng.lya_shoot(SEED, 0, 1)
    eng.close()


# ----------------------------------------------------------- refusals --

def test_refusals(small):
    from cmacionize_amd import engine as E
    import ctypes as C
    scene, eng = small
    m = scene.m
    lib, h = eng._lib, eng._h
    p = Y._p
    untouched = np.full((m.nx, m.ny), -7.)
    cube = np.full((scene.nchan, m.nx, m.ny), -7.)

    def refused(code, rc):
        assert rc == code, (rc, lib.cmi_gpu_last_error())
        assert np.all(untouched == -7.) and np.all(cube == -7.)

    def set_mode(*a):
        return lib.cmi_gpu_set_lyman_alpha(h, *a, p(scene.n_HI), p(scene.T))

    ok = (16, -1e5, 1e5, 0., 0., 1000)
    try:
        # bad arguments: the mode that is set stays
        for bad in ((-1,) + ok[1:], (16, 1e5, -1e5) + ok[3:],
                    (16, float("nan"), 1e5) + ok[3:],
                    ok[:3] + (-1.,) + ok[4:], ok[:3] + (float("nan"),) +
                    ok[4:], ok[:4] + (-3.,) + ok[5:],
                    ok[:4] + (float("nan"),) + ok[5:], ok[:5] + (0,),
                    ok[:5] + (100000001,)):
            refused(Y.EINVAL, set_mode(*bad))
        negative = scene.n_HI.copy()
        negative[3] = -1.
        refused(Y.EINVAL, lib.cmi_gpu_set_lyman_alpha(h, *ok, p(negative),
                                                      p(scene.T)))
        cold = np.zeros(m.n)
        refused(Y.EINVAL, lib.cmi_gpu_set_lyman_alpha(h, *ok, p(scene.n_HI),
                                                      p(cold)))
        assert lib.cmi_gpu_download_lya_view(h, 0, p(untouched), None) == 0
        assert np.all(untouched == 0.)
        untouched[:] = -7.
        refused(Y.EINVAL, lib.cmi_gpu_download_lya_view(h, 1, p(untouched),
                                                        p(cube)))
        # a stale mode: the camera, the source, the velocities
        for stale in (
                lambda: eng.set_ccd_image(m.theta, m.phi, m.nx, m.ny,
                                          m.img_anchor, m.img_sides),
                lambda: eng.set_cell_source_field(scene.field),
                lambda: eng.set_cell_velocities(scene.velocity)):
            scene.apply(eng)
            stale()
            refused(Y.ESTATE, lib.cmi_gpu_lya_shoot(h, 1, 0, 10))
            refused(Y.ESTATE, lib.cmi_gpu_download_lya_view(
                h, 0, p(untouched), p(cube)))
            out = np.full((1, 2), -7.)
            assert lib.cmi_gpu_lya_probe(h, Y.SAMPLER, 1, 0, 1,
                                         p(np.ones((1, 2))), p(out),
                                         0) == Y.ESTATE
            assert np.all(out == -7.)
        # a capped packet: the download fails
        eng.set_lyman_alpha(16, -1e5, 1e5, 0., 0., 2, scene.n_HI, scene.T)
        eng.lya_shoot(SEED, 0, 100)
        assert eng.get_lya_counters()["ncapped"] > 0
        refused(Y.ESTATE, lib.cmi_gpu_download_lya_view(h, 0, p(untouched),
                                                        p(cube)))
        # the mode off
        eng.set_lyman_alpha(0, 0., 1.)
        refused(Y.ESTATE, lib.cmi_gpu_lya_shoot(h, 1, 0, 10))
        refused(Y.ESTATE, lib.cmi_gpu_download_lya_view(h, 0, p(untouched),
                                                        p(cube)))
        # a point camera
        eng.set_sky_camera(m.anchor + 0.5 * m.sides, 8, 4,
                           float(m.sides.min()) / 50.)
        refused(Y.ESTATE, set_mode(*ok))
    finally:
        eng.set_ccd_image(m.theta, m.phi, m.nx, m.ny, m.img_anchor,
                          m.img_sides)
        scene.apply(eng)
    # no source; a block of a decomposed grid
    fresh = E.GpuEngine(tuple(int(v) for v in m.ncell), tuple(m.anchor),
                        tuple(m.sides), (0, 0, 0), device=0)
    fresh.upload_cells(m.density, scene.T, None)
    fresh.set_ccd_image(m.theta, m.phi, m.nx, m.ny, m.img_anchor, m.img_sides)
    refused(Y.ESTATE, lib.cmi_gpu_set_lyman_alpha(fresh._h, *ok,
                                                  p(scene.n_HI), p(scene.T)))
    fresh.close()
    block = E.GpuEngine((8, 4, 4), (0., 0., 0.), (1., 1., 1.), (0, 0, 0),
                        device=0, sub_offset=(4, 0, 0), sub_ncell=(4, 4, 4))
    block.upload_cells(np.full(64, 1e8), np.full(64, 100.),
                       np.ones((E.NION, 64)))
    refused(Y.ESTATE, lib.cmi_gpu_set_lyman_alpha(block._h, *ok, None, None))
    assert b"decomposed" in lib.cmi_gpu_last_error()
    block.close()
