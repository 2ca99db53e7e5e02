"""The CPU restatement of the Lyman-alpha transfer
(tests/support/lyman_alpha_reference.c) on its own - no GPU. It is held to
what follows from the contract (include/cmi_gpu.h, "Lyman alpha"): the Voigt
approximation against the exact function, the atom sampler against the exact
density, the identities of the cube, the thin Gaussian line without H I, the
Galilean shift, and Dijkstra et al. (2006)'s static sphere. The GPU tests
(test_gpu_lyman_alpha.py) then hold the device to the restatement."""
import numpy as np
import pytest

import line_cube_lib as LC
import lyman_alpha_lib as Y
import scattered_cube_lib as Q

SEED = 5
N = 3000


# -------------------------------------------------------------- Voigt --

@pytest.mark.parametrize("T", [10., 100., 1.0e4, 1.0e5])
def test_voigt_against_the_exact_function(T):
    """within 3 % for |x| <= 1000 (2.2 % measured at 10 K, plus margin)"""
    a = float(Y.voigt_parameter(Y.doppler_width(T)))
    x = np.r_[np.linspace(0., 12., 2401), np.logspace(np.log10(12.), 3., 800)]
    x = np.r_[-x[::-1], x]
    scene, _ = Y.parity_scene(ncell=(6, 5, 7))
    ref = Y.Restatement(scene)
    rows = np.stack([np.full(len(x), a), x, np.ones(len(x)),
                     np.zeros(len(x))], axis=1)
    H = ref.voigt(rows)[:, 0]
    exact = Y.exact_voigt(a, x)
    err = np.abs(H / exact - 1.)
    print("T", T, "a", a, "worst", err.max(), "at x", x[np.argmax(err)])
    assert err.max() <= 0.03
    assert np.array_equal(H, H[::-1])
    # the cut of exp(-x^2) at x^2 = 64 is below an ulp of the wing there
    assert np.exp(-64.) < 1e-16 * a / (np.sqrt(np.pi) * 64.)


def test_records():
    """b, a and kappa_0 of the contract; 5.90e-14 cm^2 per atom at 1e4 K"""
    scene, _ = Y.parity_scene(ncell=(6, 5, 7), sigma_turb=3.0e3)
    ref = Y.Restatement(scene)
    assert ref.invalid == 0
    r = ref.records()
    b = Y.doppler_width(scene.T, 3.0e3)
    assert np.allclose(r[:, 1] * b, 1., rtol=1e-14)
    assert np.allclose(r[:, 2], Y.voigt_parameter(b), rtol=1e-14)
    assert np.allclose(r[:, 0], scene.n_HI * Y.line_centre_cross_section(b),
                       rtol=1e-14)
    assert np.allclose(r[:, 3], scene.m.density * scene.m.sigma, rtol=1e-14)
    assert np.array_equal(r[:, 4:7], scene.velocity.T)
    s0 = Y.line_centre_cross_section(Y.doppler_width(1.0e4))
    assert abs(s0 * 1.0e4 / 5.90e-14 - 1.) < 2e-3


# ------------------------------------------------------- atom sampler --

DRAWS = 200000
BINS = 40


@pytest.mark.parametrize("a", [4.7e-4, 1.5e-2])
@pytest.mark.parametrize("x", [0., 1., 3., 8., -3.])
def test_atom_sampler_against_the_exact_density(x, a):
    """u_par of DRAWS streams in BINS bins of equal probability under f(u) ~
    exp(-u^2) / ((x - u)^2 + a^2) (its distribution function by the
    trapezoidal rule on a grid that resolves both the Gaussian and the
    Lorentzian). chi^2 has BINS - 1 degrees of freedom: mean BINS - 1,
    standard deviation sqrt(2 (BINS - 1)); the bound is five of those above
    the mean (a one-sided probability below 1e-5 for the ten cases)."""
    scene, _ = Y.parity_scene(ncell=(6, 5, 7))
    ref = Y.Restatement(scene)
    out, _ = ref.sampler(SEED, 0, np.tile([x, a], (DRAWS, 1)))
    u = out[:, 0]
    grid = np.unique(np.r_[np.linspace(-8., 8., 32001),
                           x + a * np.tan(np.linspace(-1.57, 1.57, 20001))])
    grid = grid[(grid >= -8.) & (grid <= max(8., abs(x) + 8.))]
    f = np.exp(-grid * grid) / ((x - grid) ** 2 + a * a)
    cdf = np.r_[0., np.cumsum(0.5 * (f[1:] + f[:-1]) * np.diff(grid))]
    cdf /= cdf[-1]
    edges = np.interp(np.arange(1, BINS) / BINS, cdf, grid)
    counts = np.bincount(np.searchsorted(edges, u), minlength=BINS)
    expected = DRAWS / BINS
    chi2 = float(((counts - expected) ** 2).sum() / expected)
    dof = BINS - 1
    print("x", x, "a", a, "chi2", chi2, "rejections per draw",
          out[:, 1].mean())
    assert chi2 <= dof + 5. * np.sqrt(2. * dof)
    # the separation point changes the acceptance rate only: the header's
    # worst acceptance of 0.046 is 21 rejections per draw
    assert out[:, 1].mean() < 25.


# --------------------------------------------------------- identities --

def test_one_covering_channel_is_the_image():
    scene, _ = Y.parity_scene(nchan=1, vmin=-1.0e7, vmax=1.0e7)
    image, cube, c, _ = Y.Restatement(scene).shoot(SEED, 0, N)
    assert c["nhydrogen"] > 10 * N and c["ndust"] > 0 and c["ncapped"] == 0
    assert c["npackets"] == N
    assert np.array_equal(cube[0], image)


@pytest.mark.parametrize("nchan", [5, 16])
def test_covering_channels_sum_to_the_image(nchan):
    """every event is in exactly one channel: the sums differ by the order
    of their terms only"""
    scene, _ = Y.parity_scene(nchan=nchan, vmin=-1.0e7, vmax=1.0e7)
    image, cube, c, _ = Y.Restatement(scene).shoot(SEED, 0, N)
    assert np.allclose(cube.sum(axis=0), image, rtol=1e-12, atol=0.)
    # a narrower axis resolves the line, and loses nothing it covers
    scene, _ = Y.parity_scene(nchan=nchan, vmin=-2.0e5, vmax=2.0e5)
    image2, cube2, _, _ = Y.Restatement(scene).shoot(SEED, 0, N)
    assert np.allclose(image2, image, rtol=1e-12, atol=0.)
    assert np.count_nonzero(cube2.sum(axis=(1, 2))) >= 4
    assert np.all(cube2.sum(axis=0) <= image * (1. + 1e-12))


def test_without_hydrogen_and_dust_it_is_the_thin_gaussian_line():
    """n_HI = 0, no dust: only the direct light, exp(-0) / (4 pi) per packet
    at u = -dot3(w_e, d) with w_e Gaussian of width b about the cell's
    velocity: per pixel and channel the expectation is the ray-traced cube of
    line_cube_reference.c (8 x 8 samples per pixel). Judged by z-scores from
    the restatement's own squared addends, as test_scattered_cube_host.py's
    _judge does: elements with at least 100 contributions, z <= 5, rms of
    order one."""
    scene, box = Y.parity_scene(nchan=8, vmin=-3.2e4, vmax=3.2e4, nx=10,
                                ny=10, dust=False)
    scene.n_HI[:] = 0.
    ref = Y.Restatement(scene)
    n = 800000
    image, cube, c, _, squares, hits = ref.shoot(11, 0, n, True)
    assert c["nhydrogen"] == 0 and c["ndust"] == 0
    m = scene.m
    scale = ref.total_luminosity() / (n * m.pixel_area)
    widths = Y.doppler_width(scene.T)
    rt = LC.render(box, scene.field, widths, m.theta, m.phi, m.nx, m.ny,
                   m.img_anchor, m.img_sides, scene.nchan, scene.vmin,
                   scene.vmax, 8, velocity=scene.velocity)[0]
    lit = rt > 1e-6 * rt.max()
    judged = lit & (hits >= 100)
    print("lit", lit.sum(), "judged", judged.sum())
    assert lit.sum() > 100 and judged.sum() >= 0.75 * lit.sum()
    z = np.abs(cube * scale - rt)[judged] / (np.sqrt(squares) * scale)[judged]
    print("worst", z.max(), "rms", np.sqrt(np.mean(z ** 2)))
    assert z.max() <= 5.
    assert 0.5 < np.sqrt(np.mean(z ** 2)) < 1.5


def test_galilean_shift():
    """adding V to every velocity, with dot3(V, n) = 3 channels, moves the
    cube 3 channels towards the blue: u changes by -dot3(V, n) and nothing
    else but rounding (every x is a difference of velocities)"""
    scene, _ = Y.parity_scene(nchan=20, vmin=-2.0e5, vmax=2.0e5)
    _, cube, _, _ = Y.Restatement(scene).shoot(SEED, 0, N)
    m = scene.m
    n = np.array([np.sin(m.theta) * np.cos(m.phi),
                  np.sin(m.theta) * np.sin(m.phi), np.cos(m.theta)])
    dv = (scene.vmax - scene.vmin) / scene.nchan
    V = 3. * dv * n + 1.7e4 * np.cross(n, [0., 0., 1.])
    assert abs(V @ n / dv - 3.) < 1e-12
    moved, _ = Y.parity_scene(nchan=20, vmin=-2.0e5, vmax=2.0e5)
    moved.velocity = Y._f64(scene.velocity + V[:, None])
    _, cube2, _, _ = Y.Restatement(moved).shoot(SEED, 0, N)
    assert np.allclose(cube2[:-3], cube[3:], rtol=1e-9,
                       atol=1e-12 * cube.max())
    assert cube[3:].sum() > 0.9 * cube.sum()


# ------------------------------------------------------ static sphere --

def test_static_sphere():
    """The emergent spectrum of a uniform static sphere with a tau_0 = 1000
    (lyman_alpha_lib.sphere_scene) against Dijkstra et al. (2006)'s J(x): the
    median of |x| is 8.98 there; an independent gridless Monte Carlo of this
    case gave 9.15, and the formula is asymptotic: within 5 %. The blue share
    of the flux is within 4 binomial standard errors of 1 / 2."""
    scene, b, a = Y.sphere_scene()
    expected = Y.static_sphere_median(Y.SPHERE_A_TAU0)
    assert abs(expected - 8.98) < 0.01
    ref = Y.Restatement(scene)
    n = Y.SPHERE_PACKETS
    image, cube, c, _ = ref.shoot(Y.SPHERE_SEED, 0, n)
    assert c["ncapped"] == 0 and c["ndust"] == 0
    median, blue = Y.sphere_statistics(cube, scene, b)
    print("median |x|", median, "expected", expected, "blue share", blue,
          "scatterings per packet", c["nhydrogen"] / n,
          "flux inside the axis", cube.sum() / image.sum())
    assert cube.sum() > 0.999 * image.sum()
    assert abs(median / expected - 1.) <= 0.05
    assert abs(blue - 0.5) <= 4. * np.sqrt(0.25 / n)


# ------------------------------------------- the GPU tests' own seeds --

def test_parity_seeds_need_no_excuse():
    """the traces that test_gpu_lyman_alpha.py compares row by row: no
    decision (species, rejection) of those packets within 1e-9 of its
    threshold, no event on a cell wall, no velocity within 1e-9 channels of a
    channel edge - the GPU test leaves no row out"""
    scene, _ = Y.parity_scene()
    ref = Y.Restatement(scene)
    trace, margins = ref.trace(Y.TRACE_SEED, 0, Y.TRACE_PACKETS,
                               Y.TRACE_EVENTS)
    assert margins.min() > 1e-9
    rows, _ = Y.events(_clip(trace, Y.TRACE_EVENTS), Y.TRACE_EVENTS)
    assert not Q.near_wall(scene.m, rows[:, 0:3]).any()
    f = (rows[:, 9] - scene.vmin) / ((scene.vmax - scene.vmin) / scene.nchan)
    assert np.abs(f - np.round(f)).min() > 1e-9
    # tens to hundreds of scatterings, both species
    per_packet = trace[:, 1] + trace[:, 2]
    print("scatterings per packet: median", np.median(per_packet), "max",
          per_packet.max())
    assert np.median(per_packet) >= 10 and trace[:, 2].sum() > 0


def _clip(trace, cap):
    """a trace whose event counts are cut at the rows it holds"""
    out = trace.copy()
    out[:, 0] = np.minimum(out[:, 0], cap)
    return out


# -------------------------------------------------------------- driver --

import os  # noqa: E402
import subprocess  # noqa: E402

import scattered_line_lib as SL  # noqa: E402

GOLDEN = os.path.join(SL.HERE, "golden", "multi_view")
ONE_VIEW = open(os.path.join(GOLDEN, "one_view_lines.param")).read()
IMAGES, SKY = ONE_VIEW.split("EmissionSkyMaps:\n")
SKY = "EmissionSkyMaps:\n" + SKY
CHANNELS = ("  velocity channels: 8\n  velocity minimum: -40. km s^-1\n"
            "  velocity maximum: 40. km s^-1\n")
KEY = "  Lyman alpha: %s\n"


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
     "EmissionImages:Lyman alpha needs velocity channels"),
    (IMAGES + "  type: PGM\n" + CHANNELS + KEY % "true" + SKY,
     "needs type BinaryArray"),
    (IMAGES + CHANNELS + KEY % "true" +
     "  Lyman alpha core skipping: -1.\n" + SKY,
     "EmissionImages:Lyman alpha core skipping must not be negative"),
    (IMAGES + CHANNELS + KEY % "true" +
     "  Lyman alpha maximum scatterings: 0\n" + SKY,
     "EmissionImages:Lyman alpha maximum scatterings must be 1..100000000"),
    (IMAGES + CHANNELS + KEY % "true" +
     "  Lyman alpha maximum scatterings: 100000001\n" + SKY,
     "EmissionImages:Lyman alpha maximum scatterings must be 1..100000000"),
    (IMAGES.replace("  scattering: true\n", "").replace(
        "packets: 20000", "packets: 0") + CHANNELS + KEY % "true" + SKY,
     "EmissionImages:number of packets must be positive"),
    (IMAGES + SKY + CHANNELS + KEY % "true",
     "EmissionSkyMaps:Lyman alpha is not supported"),
])
def test_driver_refuses(tmp_path, text, message):
    r, used = _emission(tmp_path, text)
    assert r.returncode != 0 and message in r.stderr, r.stderr
    assert "Could not open" not in r.stderr
    assert not os.path.exists(used)


def test_driver_accepts_the_key_and_lists_it(tmp_path):
    text = IMAGES + CHANNELS + KEY % "true" + \
        "  Lyman alpha core skipping: 5.\n" + SKY
    r, used = _emission(tmp_path, text, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    used = open(used).read()
    assert used.count("Lyman alpha: true") == 1
    assert "Lyman alpha core skipping: 5" in used
    assert "Lyman alpha maximum scatterings: 100000000" in used


def test_driver_without_the_key_reads_nothing_new(tmp_path):
    """with the key absent the used-values are what they were (the golden
    file); with the key false it is listed as not used and nothing else
    changes"""
    r, used = _emission(tmp_path, ONE_VIEW, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    assert open(used).read() == \
        open(os.path.join(GOLDEN, "one_view_lines.param.usedvalues")).read()
    text = IMAGES + CHANNELS + SKY
    r, used = _emission(tmp_path, text, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    absent = open(used).read()
    assert "Lyman alpha" not in absent
    text = IMAGES + CHANNELS + KEY % "false" + SKY
    r, used = _emission(tmp_path, text, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    off = open(used).read()
    assert off.count("Lyman alpha: value not used") == 1
    assert [l for l in off.split("\n") if "Lyman alpha" not in l] == \
        absent.split("\n")
