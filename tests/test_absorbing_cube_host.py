"""Absorbing line cubes without a GPU: the CPU restatement
(tests/support/absorbing_cube_reference.c) against closed forms and the
contract's exact identities, the 21-cm constants and limits, the keys of
`cmi-gpu --emission` up to the point where it opens the snapshot, and what is
refused before a device is needed."""
import os
import re
import subprocess
from decimal import Decimal, getcontext

import numpy as np
import pytest

import absorbing_cube_lib as A
import continuum_lib as K
import line_cube_lib as LC
import line_image_lib as L
import scattered_line_lib as SL

BOX, NX, NY = A.BOX, A.NX, A.NY
GOLDEN = os.path.join(L.HERE, "golden", "multi_view")
EPS = np.finfo(np.float64).eps


def axis_view(axis):
    """the view along +axis and the box's depth along it"""
    theta, phi = [(LC.HALF, 0.), (LC.HALF, LC.HALF), (0., 0.)][axis]
    return theta, phi, BOX.sides[axis]


# ------------------------------------------------------- the restatement --

@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("peak", [1e-4, 1., 60.])
def test_uniform_slab(axis, peak):
    """I_c = S (1 - exp(-a f_c L / dv)) + bg exp(-a f_c L / dv) along an
    axis, for a thin line, tau ~ 1 and tau > 40 at the centre; rays that miss
    return bg"""
    theta, phi, depth = axis_view(axis)
    anchor, sides = A.image_rectangle(BOX, theta, phi)
    nchan, b, S, bg = 7, 3., 2.5, 0.75
    vmin, vmax = -10.5, 10.5
    dv = (vmax - vmin) / nchan
    f = LC.fractions(nchan, vmin, vmax, 0., b)
    a = peak * dv / (depth * f.max())
    got = A.cube(BOX, a * np.ones(BOX.n), S * np.ones(BOX.n),
                 b * np.ones(BOX.n), theta, phi, NX, NY, anchor, sides, nchan,
                 vmin, vmax, 2, background=bg)
    tau = a * f * depth / dv
    assert abs(tau.max() / peak - 1.) < 1e-12
    want = S * -np.expm1(-tau) + bg * np.exp(-tau)
    xy = L.sample_coordinates(NX, NY, anchor, sides, 2)
    chord = L.chords(BOX, theta, phi, xy.reshape(-1, 2)).reshape(NX, NY, 4)
    hit, miss = (chord > 0.).all(axis=2), (chord == 0.).all(axis=2)
    assert hit.sum() > 0.5 * NX * NY and miss.sum() > 20
    assert np.array_equal(got[:, miss], np.full((nchan, miss.sum()), bg))
    cells = BOX.ncell[axis]
    depth_of_line = A.line_depth(BOX, a, dv)
    for c in range(nchan):
        err = np.abs(got[c][hit] - want[c]).max()
        # per cell the bound of the parity tests covers the restatement
        # against exact arithmetic as well; the sum of the cells' tau has 2
        # eps per cell of its own, numpy's exp and expm1 an ulp each
        allowed = A.march_bound(cells, depth_of_line, [S], None, [bg],
                                supersample=2) + \
            (2 * cells * tau[c] + 4) * EPS * max(S, bg)
        assert err <= allowed, (c, err, allowed)


def test_exact_identities():
    """a == 0: every channel is the continuum image of {kc, sc}, bit for bit,
    for both cameras; sl == sc == bg stays bg whatever the opacities are; a
    channel does not depend on how many channels the cube has"""
    a, sl, b, vel, kc, sc = A.random_cells(BOX, 5, 2.)
    bg = 0.7 * sl.mean()
    nchan, vmin, vmax = 5, -4., 6.
    d = A.sky_directions()
    for theta, phi in A.VIEWS:
        anchor, sides = A.image_rectangle(BOX, theta, phi)
        want = K.images(BOX, kc, sc, theta, phi, NX, NY, anchor, sides,
                        background=bg)
        got = A.cube(BOX, np.zeros(BOX.n), sl, b, theta, phi, NX, NY, anchor,
                     sides, nchan, vmin, vmax, velocity=vel, kc=kc, sc=sc,
                     background=bg)
        for c in range(nchan):
            assert np.array_equal(got[c], want[0]), (theta, phi, c)
        flat = np.full(BOX.n, bg)
        got = A.cube(BOX, a, flat, b, theta, phi, NX, NY, anchor, sides,
                     nchan, vmin, vmax, velocity=vel, kc=kc, sc=flat,
                     background=bg)
        assert np.array_equal(got, np.full(got.shape, bg))
        # the first channels of a cube twice as long
        one = A.cube(BOX, a, sl, b, theta, phi, NX, NY, anchor, sides, 4,
                     vmin, vmin + 8., velocity=vel, kc=kc, sc=sc,
                     background=bg)
        two = A.cube(BOX, a, sl, b, theta, phi, NX, NY, anchor, sides, 8,
                     vmin, vmin + 16., velocity=vel, kc=kc, sc=sc,
                     background=bg)
        assert np.array_equal(one, two[:4])
        assert len(np.unique(one)) > 100
    for origin in A.sky_origins(BOX):
        want = K.sky(BOX, kc, sc, origin, d, background=bg)
        got = A.sky_cube(BOX, np.zeros(BOX.n), sl, b, origin, d, nchan, vmin,
                         vmax, velocity=vel, kc=kc, sc=sc, background=bg,
                         observer_velocity=(1., -2., 0.5))
        for c in range(nchan):
            assert np.array_equal(got[c], want[0])


def test_sky_form_agrees_with_the_parallel_form_from_far_away():
    """rays from a distant origin through the pixel centres of a view are the
    parallel camera's rays up to the angle they subtend; a uniform velocity
    has the same radial component for both"""
    dv = 2.
    a, sl, b, vel, kc, sc = A.random_cells(BOX, 9, dv, tau_lo=1e-3, tau_hi=3.)
    # smooth fields, so that a slightly different path changes little
    # (and a line source function well above the continuum's)
    a[:], kc[:], sl[:], sc[:] = a.mean(), kc.mean(), sl.mean(), 0.3 * sl.mean()
    b[:] = 3.
    theta, phi = 0.7, 0.3
    n, ex, ey = L.axes(theta, phi)
    vel = np.outer([30., -10., 20.], np.ones(BOX.n))
    u = -(vel[:, 0] @ n)
    nchan, vmin, vmax = 6, u - 6., u + 6.
    anchor, sides = L.bounding_rectangle(BOX, theta, phi)
    nx, ny = 6, 5
    flat = A.cube(BOX, a, sl, b, theta, phi, nx, ny, anchor, sides, nchan,
                  vmin, vmax, velocity=vel, kc=kc, sc=sc, background=sl[0])
    xy = L.sample_coordinates(nx, ny, anchor, sides).reshape(-1, 2)
    origin = 1e7 * n
    d = xy[:, :1] * ex + xy[:, 1:] * ey - origin
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    seen = A.sky_cube(BOX, a, sl, b, origin, d, nchan, vmin, vmax,
                      velocity=vel, kc=kc, sc=sc,
                      background=sl[0]).reshape(nchan, nx, ny)
    assert np.abs(seen - flat).max() <= 1e-4 * max(sl.max(), sc.max())
    assert np.abs(seen - flat).max() > 0.
    # the line is there: the channels differ
    assert np.abs(flat[2] - flat[0]).max() > 1e-2 * sl.max()


def test_probe_rows_are_the_render():
    dv = 2.
    a, sl, b, vel, kc, sc = A.random_cells(BOX, 21, dv)
    theta, phi = A.VIEWS[3]
    anchor, sides = A.image_rectangle(BOX, theta, phi)
    xy = L.sample_coordinates(NX, NY, anchor, sides).reshape(-1, 2)
    rows = A.probe(BOX, a, sl, b, xy, 40, 5, -4., 6., theta=theta, phi=phi,
                   velocity=vel, kc=kc, sc=sc, background=sl[0])
    t, steps, cells, ds, I, I_end = A.split_probe(rows, 5, 40)
    img = A.cube(BOX, a, sl, b, theta, phi, NX, NY, anchor, sides, 5, -4., 6.,
                 velocity=vel, kc=kc, sc=sc, background=sl[0])
    assert np.array_equal(I_end.T.reshape(5, NX, NY), img)
    geometry = L.probe(BOX, theta, phi, xy, 40)
    assert np.array_equal(rows[:, :3 + 80], geometry, equal_nan=True)
    assert steps.max() <= 40 and steps.max() == A.longest_ray


# --------------------------------------------------------- the 21-cm line --

def test_column_constant():
    """C_HI recomputed from the constants with 40 digits, and against the
    textbook's N_HI = 1.813e18 cm^-2 per K km s^-1"""
    from cmacionize_amd import engine as E
    getcontext().prec = 40
    h, k, c = Decimal("6.626070040e-34"), Decimal("1.38064852e-23"), \
        Decimal(299792458)
    A10, nu = Decimal("2.8843e-15"), Decimal("1420405751.768")
    pi = Decimal("3.141592653589793238462643383279502884197")
    C_HI = float(3 * h * c ** 3 * A10 / (32 * pi * k * nu * nu))
    assert E.HI_FREQUENCY == float(nu) and E.HI_EINSTEIN_A == float(A10)
    assert (E.PLANCK, E.BOLTZMANN, E.LIGHTSPEED) == \
        (float(h), float(k), float(c))
    for value in (E.HI_COLUMN_CONSTANT, A.HI_COLUMN_CONSTANT):
        assert abs(value / C_HI - 1.) < 1e-12
    assert abs(E.HI_COLUMN_CONSTANT * (1.813e18 * 1e4 * 1e-3) - 1.) < 1e-3
    # the same literal in the device code
    text = open(os.path.join(L.ROOT, "cmacionize_amd", "csrc",
                             "device_common.h")).read()
    literal = re.search(r"#define CMI_HI_COLUMN_CONSTANT (\S+)", text).group(1)
    assert float(literal) == E.HI_COLUMN_CONSTANT


def hi_slab(T_s, peak_tau, sigma_turb=0.):
    """a static uniform neutral slab, seen along z: its coefficients, the
    column density, and a velocity axis that holds the whole line"""
    depth = BOX.sides[2]
    b = np.sqrt(2. * (A.BOLTZMANN * T_s /
                      (A.HYDROGEN_WEIGHT * A.ATOMIC_MASS_UNIT) +
                      sigma_turb ** 2))
    column = peak_tau * np.sqrt(np.pi) * b * T_s / A.HI_COLUMN_CONSTANT
    n = column / depth
    q = A.hi_coefficients(n * np.ones(BOX.n), T_s * np.ones(BOX.n),
                          np.ones(BOX.n), np.ones(BOX.n), 0.1,
                          sigma_turb=sigma_turb)
    assert abs(q["b"][0] / b - 1.) < 1e-15 and not q["kc"].any()
    return q, column, (-8. * b, 8. * b)


def test_thin_column():
    """sum_c T_b,c dv gives N_HI within 1e-3 where the line is thin: the
    error is tau / 2 of the peak (less over the whole profile) and the
    Rayleigh-Jeans term h nu / (2 k T_s), and the slab is chosen inside it"""
    from cmacionize_amd import engine as E
    T_s, peak = 100., 5e-4
    x = A.PLANCK * A.HI_FREQUENCY / (A.BOLTZMANN * T_s)
    assert 0.5 * peak + 0.5 * x < 1e-3
    q, column, (vmin, vmax) = hi_slab(T_s, peak)
    theta, phi, _ = axis_view(2)
    anchor, sides = L.bounding_rectangle(BOX, theta, phi)
    nchan = 32
    cube = A.cube(BOX, q["a"], q["sl"], q["b"], theta, phi, 3, 2, anchor,
                  sides, nchan, vmin, vmax)
    got = E.hi_column_density(cube, (vmax - vmin) / nchan)
    assert got.shape == (3, 2)
    assert np.abs(got / column - 1.).max() < 1e-3
    assert (got < column).all()     # both terms take away


def test_thick_limit():
    """tau > 40 across the band: I is B_nu(T_s) to rounding, whatever is
    behind, and the Rayleigh-Jeans T_b is T_s less h nu / 2 k"""
    from cmacionize_amd import engine as E
    T_s = 80.
    q, column, _ = hi_slab(T_s, 1e4)
    theta, phi, _ = axis_view(2)
    anchor, sides = L.bounding_rectangle(BOX, theta, phi)
    half = 2. * q["b"][0]       # f_c e^-4 of the peak at the band's ends
    cube = A.cube(BOX, q["a"], q["sl"], q["b"], theta, phi, 3, 2, anchor,
                  sides, 8, -half, half, background=A.host_planck(5000.))
    B = A.planck(A.HI_FREQUENCY, np.array([T_s]))[0]
    assert np.abs(cube / B - 1.).max() <= 4 * EPS
    T_b = E.brightness_temperature(cube, E.HI_FREQUENCY)
    shift = 0.5 * A.PLANCK * A.HI_FREQUENCY / A.BOLTZMANN
    assert np.abs(T_b - (T_s - shift)).max() < 1e-5


@pytest.mark.parametrize("cold_in_front", [True, False])
def test_absorption_against_the_continuum(cold_in_front):
    """cold H I (T_s = 100 K) in front of a free-free slab of 8000 K and
    T_b ~ 800 K shows a dip below the continuum at the line centre; behind
    the slab it shows none"""
    from cmacionize_amd import engine as E
    box = L.Box((0., 0., 0.), (3e16, 3e16, 3e16), (3, 3, 8))
    front = np.zeros(tuple(box.ncell), dtype=bool)
    front[:, :, 4:] = True          # the observer is at +z
    front = front.reshape(-1)
    cold = front if cold_in_front else ~front
    n = np.where(cold, 2.8e8, 1e9)
    T = np.where(cold, 100., 8000.)
    x0 = np.where(cold, 1., 0.)
    q = A.hi_coefficients(n, T, x0, x0, 0.1)
    assert not q["a"][~cold].any() and not q["kc"][cold].any()
    b = q["b"][cold][0]
    nchan = 21
    anchor, sides = L.bounding_rectangle(box, 0., 0.)
    cube = A.cube(box, q["a"], q["sl"], q["b"], 0., 0., 1, 1, anchor, sides,
                  nchan, -10.5 * b, 10.5 * b, kc=q["kc"], sc=q["sc"])
    T_b = E.brightness_temperature(cube[:, 0, 0], E.HI_FREQUENCY)
    continuum, centre = T_b[0], T_b[nchan // 2]
    assert T_b[0] == T_b[-1] and 500. < continuum < 1200.
    tau = q["a"][cold][0] * 1.5e16 / (np.sqrt(np.pi) * b)
    assert 0.5 < tau < 2.
    if cold_in_front:
        assert centre < continuum - 100.
        assert (T_b <= continuum).all()
    else:
        assert (T_b >= continuum).all() and centre > continuum + 10.


def test_special_cells():
    """n_HI == 0, T <= 0 or T_s <= 0: a == 0 exactly, and nothing is NaN"""
    n = [0., 1e8, 1e8, 1e8, 1e8]
    T = [100., 100., 0., -5., 100.]
    x0 = [1., 0., 1., 1., 1.]
    with np.errstate(all="raise"):
        q = A.hi_coefficients(n, T, x0, x0, 0.1, sigma_turb=10.)
    assert not q["a"][:4].any() and q["a"][4] > 0.
    assert (q["b"][2:4] == np.sqrt(2. * 100.)).all()
    assert all(np.isfinite(v).all() for v in q.values())
    q = A.hi_coefficients(n, T, x0, x0, 0.1,
                          spin_temperature=[50., 50., 50., 50., 0.])
    assert not q["a"].any() and q["sl"][4] == 0. and q["sl"][0] > 0.


# ---------------------------------------------------------------- plumbing --

SYMBOLS = ("cmi_gpu_hi_coefficients", "cmi_gpu_render_hi_cube",
           "cmi_gpu_render_hi_sky_cube", "cmi_gpu_render_hi_sky_map_cube",
           "cmi_gpu_render_field_absorbing_cube",
           "cmi_gpu_render_field_absorbing_sky_cube",
           "cmi_gpu_absorbing_cube_probe")


def test_symbols_and_methods():
    from cmacionize_amd import engine as E
    header = open(os.path.join(L.ROOT, "include", "cmi_gpu.h")).read()
    for name in SYMBOLS:
        assert name in E.EXPORTED_SYMBOLS
        assert re.search(r"\b%s\(" % name, header)
        assert hasattr(E.load_library(), name)
        assert callable(getattr(E.GpuEngine, name[len("cmi_gpu_"):]))
    cube = np.ones((4, 2, 3))
    T_b = E.brightness_temperature(1., E.HI_FREQUENCY)
    assert np.allclose(E.hi_column_density(cube, 500.),
                       4 * T_b * 500. / E.HI_COLUMN_CONSTANT, rtol=1e-15)


def test_refusals_that_need_no_device():
    """null pointers are refused by the C ABI before anything is touched"""
    from cmacionize_amd import engine as E
    lib = E.load_library()
    out = np.zeros(4)
    p = A._p(out)
    assert lib.cmi_gpu_hi_coefficients(None, 0., 0, None, 1, p, p, p, p,
                                       p) != 0
    assert b"hi_coefficients: null argument" in lib.cmi_gpu_last_error()
    assert lib.cmi_gpu_render_hi_cube(None, 0., 0., 1, 1, p, p, 1, 1, 0., 1.,
                                      0., 0, None, 1, 0., p) != 0
    assert b"render_hi_cube: null argument" in lib.cmi_gpu_last_error()
    assert lib.cmi_gpu_render_hi_sky_cube(None, p, None, 1, p, 1, 0., 1., 0.,
                                          0, None, 1, 0., p) != 0
    assert b"render_hi_sky_cube: null argument" in lib.cmi_gpu_last_error()
    assert lib.cmi_gpu_render_hi_sky_map_cube(
        None, p, p, 0., 1., 0., 1., 1, 1, None, 1, 0., 1., 0., 0, None, 1,
        0., p) != 0
    assert b"render_hi_sky_map_cube: null argument" in \
        lib.cmi_gpu_last_error()
    assert lib.cmi_gpu_render_field_absorbing_cube(
        None, p, p, p, None, None, None, None, 0., 0., 1, 1, p, p, 1, 1, 0.,
        1., p) != 0
    assert b"render_field_absorbing_cube: null argument" in \
        lib.cmi_gpu_last_error()
    assert lib.cmi_gpu_render_field_absorbing_sky_cube(
        None, p, p, p, None, None, None, None, p, None, 1, p, 1, 0., 1.,
        p) != 0
    assert b"render_field_absorbing_sky_cube: null argument" in \
        lib.cmi_gpu_last_error()
    assert lib.cmi_gpu_absorbing_cube_probe(
        None, p, p, p, None, None, None, None, 1, 0., 1., 0, p, None, 1, p,
        4, p) != 0
    assert b"absorbing_cube_probe: bad argument" in lib.cmi_gpu_last_error()


# ------------------------------------------------- the kernels' figures --

# VGPRs and waves per SIMD of the march kernels <CB, CALL> (gfx950, the
# Makefile's flags; DESIGN.md 4.16 quotes them)
MARCH_FIGURES = {("cube", 4, 1): (80, 6), ("cube", 4, 0): (101, 4),
                 ("cube", 8, 1): (104, 4), ("cube", 8, 0): (125, 4),
                 ("sky", 4, 1): (109, 4), ("sky", 4, 0): (130, 3),
                 ("sky", 8, 1): (149, 3), ("sky", 8, 0): (170, 2)}


def test_march_kernels_static_figures():
    """from the kernels' metadata in the compiler's listing (`make asm`,
    made again if a source of the library is newer than it): no march kernel
    of any variant has a private segment, each has the VGPRs stated above,
    and they fit the stated waves per SIMD (512 / waves, in granules of 8)"""
    csrc = os.path.join(L.ROOT, "cmacionize_amd", "csrc")
    listing = os.path.join(csrc, "engine.s")
    sources = [os.path.join(csrc, name) for name in os.listdir(csrc)
               if name.endswith((".h", ".hip"))]
    sources.append(os.path.join(L.ROOT, "include", "cmi_gpu.h"))
    if not os.path.exists(listing) or os.path.getmtime(listing) < max(
            os.path.getmtime(path) for path in sources):
        subprocess.run(["make", "-C", csrc, "asm"], check=True)
    text = open(listing).read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = set()
    for entry in re.split(r"\n  - ", meta):
        name = re.search(r"\.name:\s+(\S+)", entry)
        m = name and re.search(
            r"absorbing_(sky|cube)_march_kernelILi(\d+)ELb([01])E",
            name.group(1))
        if not m:
            continue
        key = (m.group(1), int(m.group(2)), int(m.group(3)))
        found.add(key)
        private = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)",
                                entry).group(1))
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1))
        want, waves = MARCH_FIGURES[key]
        print(name.group(1), "private segment", private, "VGPRs", vgprs,
              "stated", want, "waves", waves)
        assert private == 0
        assert vgprs == want and vgprs <= 512 // waves // 8 * 8
    assert found == set(MARCH_FIGURES)
    design = open(os.path.join(L.ROOT, "DESIGN.md")).read()
    for (kind, cb, call), (vgprs, waves) in MARCH_FIGURES.items():
        assert "`absorbing_%s_march_kernel<%d, %s>`: %d VGPRs, %d waves " \
            "per SIMD" % (kind, cb, "call" if call else "inline", vgprs,
                          waves) in design


# ------------------------------------------------------------ the driver --

ONE_VIEW = open(os.path.join(GOLDEN, "one_view_lines.param")).read()
USED = open(os.path.join(GOLDEN, "one_view_lines.param.usedvalues")).read()
PLAIN = ("EmissivityValues:\n  Halpha: true\nEmissionImages:\n"
         "  view theta: 60. degrees\n")
PLAIN_SKY = ("EmissivityValues:\n  Halpha: true\nEmissionSkyMaps:\n"
             "  observer position: [1.e16 m, 2.e16 m, -3.e16 m]\n")
AXIS = ("  velocity channels: 8\n  velocity minimum: -20. km s^-1\n"
        "  velocity maximum: 20. km s^-1\n")
KEYS = AXIS + "  HI cube: true\n"


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


@pytest.mark.parametrize("block, name", [(PLAIN, "EmissionImages"),
                                         (PLAIN_SKY, "EmissionSkyMaps")])
@pytest.mark.parametrize("more, message", [
    ("  HI cube: true\n", "%s:HI cube needs velocity channels"),
    ("  HI cube: true\n  type: PGM\n", "%s:HI cube needs type BinaryArray"),
    (KEYS + "  HI spin temperature type: Fixed\n",
     "%s:HI spin temperature is required with HI spin temperature type "
     "Fixed"),
    (KEYS + "  HI spin temperature type: Fixed\n"
     "  HI spin temperature: -100. K\n",
     "%s:HI spin temperature must be positive"),
    (KEYS + "  HI spin temperature type: Warm\n",
     "Unknown %s:HI spin temperature type \"Warm\" (Kinetic or Fixed)"),
    (KEYS + "  HI background temperature: -2.7 K\n",
     "%s:HI background temperature must not be negative"),
])
def test_driver_refuses(tmp_path, block, name, more, message):
    r, _ = _emission(tmp_path, block + more)
    assert r.returncode != 0
    assert message.replace("%s", name) in r.stderr, r.stderr
    assert "Could not open" not in r.stderr


def test_driver_reads_the_keys_only_with_the_switch(tmp_path):
    """with `HI cube: true` the used-values list the new keys; without the
    switch, or with it off, a file gives the used-values it gave before the
    keys existed and the other new keys are not read; the two blocks are read
    apart"""
    images = KEYS + ("  HI spin temperature type: Fixed\n"
                     "  HI spin temperature: 120. K\n"
                     "  HI free-free continuum: false\n"
                     "  HI background temperature: 2.725 K\n")
    text = ONE_VIEW.replace("EmissionSkyMaps:\n",
                            images + "EmissionSkyMaps:\n") + KEYS
    r, used = _emission(tmp_path, text, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    used = open(used).read()
    first, second = used.split("EmissionSkyMaps:")
    for word in ("HI cube: true", "HI spin temperature type: Fixed",
                 "HI spin temperature: 120 K",
                 "HI free-free continuum: false",
                 "HI background temperature: 2.725 K"):
        assert word in first, (word, used)
    for word in ("HI cube: true", "HI spin temperature type: Kinetic",
                 "HI free-free continuum: true",
                 "HI background temperature: 0 K"):
        assert word in second, (word, used)
    assert "HI spin temperature:" not in second
    assert "value not used" not in used
    r, used = _emission(tmp_path, ONE_VIEW, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    assert open(used).read() == USED
    r, used = _emission(
        tmp_path, ONE_VIEW + "  HI cube: false\n"
        "  HI background temperature: 3. K\n", dry_run=False)
    text = open(used).read()
    assert "HI cube: value not used" in text
    assert "HI background temperature: value not used" in text
