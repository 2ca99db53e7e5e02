"""Continuum images without a GPU: the CPU restatement
(tests/support/continuum_reference.c) against closed forms and the contract's
exact identities, the free-free formulas against the Altenhoff approximation
and their limits, the numpy helpers, the keys of `cmi-gpu --emission` up to
the point where it opens the snapshot (frequency spacing and the new units
included), and what is refused before a device is needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import continuum_lib as K
import line_image_lib as L
import scattered_line_lib as SL

BOX, NX, NY = K.BOX, K.NX, K.NY
GOLDEN = os.path.join(L.HERE, "golden", "multi_view")
EPS = np.finfo(np.float64).eps


# ------------------------------------------------------- the restatement --

def axis_view(axis):
    """the view along +axis and the box's depth along it"""
    theta, phi = [(K.LC.HALF, 0.), (K.LC.HALF, K.LC.HALF), (0., 0.)][axis]
    return theta, phi, BOX.sides[axis]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_uniform_slab(axis):
    """I = bg e^-tau + S (1 - e^-tau) along an axis, for tau from thin to
    thick; rays that miss return bg"""
    theta, phi, depth = axis_view(axis)
    anchor, sides = K.image_rectangle(BOX, theta, phi)
    tau = np.array([1e-9, 1e-3, 0.3, 1., 7., 60.])
    kappa = (tau / depth)[:, None] * np.ones(BOX.n)
    S = np.array([3., 1., 0.5, 2., 9., 4.])[:, None] * np.ones(BOX.n)
    bg = np.array([1., 2., 0., 5., 1., 100.])
    got = K.images(BOX, kappa, S, theta, phi, NX, NY, anchor, sides, 2,
                   background=bg)
    want = bg * np.exp(-tau) + S[:, 0] * -np.expm1(-tau)
    # pixels with all four samples in the box, and those with none
    xy = L.sample_coordinates(NX, NY, anchor, sides, 2)
    chord = L.chords(BOX, theta, phi, xy.reshape(-1, 2)).reshape(NX, NY, 4)
    hit, miss = (chord > 0.).all(axis=2), (chord == 0.).all(axis=2)
    assert hit.sum() > 0.5 * NX * NY and miss.sum() > 20
    assert np.array_equal(got[:, miss], np.broadcast_to(
        bg[:, None], (len(bg), miss.sum())))
    cells = BOX.ncell[axis]
    for f in range(len(tau)):
        inner = got[f][hit]
        err = np.abs(inner - want[f]).max()
        # per cell: the bound of the parity tests (18 eps of max(S, bg))
        # covers the restatement against exact arithmetic as well; the sum of
        # the cells' tau has 2 eps per cell of its own
        allowed = K.march_bound(cells, S[f], bg[f:f + 1], supersample=2) + \
            2 * cells * EPS * tau[f] * max(S[f, 0], bg[f])
        assert err <= allowed, (f, err, allowed)


def test_two_layer_slab():
    """two layers along z: the far one shines through the near one"""
    theta, phi, depth = axis_view(2)
    anchor, sides = L.bounding_rectangle(BOX, theta, phi)
    nz = BOX.ncell[2]
    near = np.zeros(tuple(BOX.ncell), dtype=bool)
    near[:, :, nz // 3:] = True     # the observer is at +z
    near = near.reshape(-1)
    t_far, t_near = 0.8, 2.5
    S_far, S_near, bg = 4., 0.25, 1.5
    d_far = depth * (nz // 3) / nz
    kappa = np.where(near, t_near / (depth - d_far), t_far / d_far)
    S = np.where(near, S_near, S_far)
    got = K.images(BOX, kappa, S, theta, phi, 5, 4, anchor, sides,
                   background=bg)
    behind = bg * np.exp(-t_far) + S_far * -np.expm1(-t_far)
    want = behind * np.exp(-t_near) + S_near * -np.expm1(-t_near)
    assert np.abs(got - want).max() <= 40 * nz * EPS * S_far


def test_exact_identities():
    """kappa == 0 leaves bg untouched; S == bg stays bg whatever kappa is -
    both bit for bit, in every view, hit or miss"""
    kappa, S, bg = K.random_channels(BOX, 3, 5)
    for theta, phi in K.VIEWS:
        anchor, sides = K.image_rectangle(BOX, theta, phi)
        got = K.images(BOX, np.zeros_like(kappa), S, theta, phi, NX, NY,
                       anchor, sides, 3, background=bg)
        # (the mean of 9 equal samples: the sum of 9 bg is not 9 * bg in
        # general, so compare at s == 1 for equality and at s == 3 to 9 eps)
        assert np.abs(got - bg[:, None, None]).max() <= 10 * EPS * bg.max()
        got = K.images(BOX, np.zeros_like(kappa), S, theta, phi, NX, NY,
                       anchor, sides, 1, background=bg)
        assert np.array_equal(got, np.broadcast_to(bg[:, None, None],
                                                   got.shape))
        flat = bg[:, None] * np.ones(BOX.n)
        got = K.images(BOX, kappa, flat, theta, phi, NX, NY, anchor, sides,
                       1, background=bg)
        assert np.array_equal(got, np.broadcast_to(bg[:, None, None],
                                                   got.shape))
    # observer outwards the same identities hold to rounding only (T and I
    # are carried apart), kappa == 0 exactly
    d = K.sky_directions()
    for origin in K.sky_origins(BOX):
        got = K.sky(BOX, np.zeros_like(kappa), S, origin, d, background=bg)
        assert np.array_equal(got, np.broadcast_to(bg[:, None], got.shape))


def test_sky_form_agrees_with_the_parallel_form_from_far_away():
    """rays from a distant origin through the pixel centres of a view are the
    parallel camera's rays up to the angle they subtend"""
    kappa, S, bg = K.random_channels(BOX, 2, 9, tau_lo=1e-3, tau_hi=3.)
    # smooth fields, so that a slightly different path changes little
    kappa[:] = kappa.mean(axis=1, keepdims=True)
    S[:] = S.mean(axis=1, keepdims=True)
    theta, phi = 0.7, 0.3
    anchor, sides = L.bounding_rectangle(BOX, theta, phi)
    nx, ny = 6, 5
    flat = K.images(BOX, kappa, S, theta, phi, nx, ny, anchor, sides,
                    background=bg)
    n, ex, ey = L.axes(theta, phi)
    xy = L.sample_coordinates(nx, ny, anchor, sides).reshape(-1, 2)
    distance = 1e7
    origin = distance * n
    target = xy[:, :1] * ex + xy[:, 1:] * ey
    d = target - origin
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    seen = K.sky(BOX, kappa, S, origin, d, background=bg).reshape(2, nx, ny)
    # path lengths differ by the relative 1e-7 the angle brings, tau <= 3 per
    # cell over <= 31 cells
    assert np.abs(seen - flat).max() <= 1e-4 * S.max()
    assert np.abs(seen - flat).max() > 0.


def test_probe_rows_are_the_render():
    kappa, S, bg = K.random_channels(BOX, 3, 21)
    theta, phi = K.VIEWS[3]
    anchor, sides = K.image_rectangle(BOX, theta, phi)
    xy = L.sample_coordinates(NX, NY, anchor, sides).reshape(-1, 2)
    rows = K.probe(BOX, kappa, S, xy, 40, theta=theta, phi=phi,
                   background=bg)
    t, steps, cells, ds, I, I_end = K.split_probe(rows, 3, 40)
    img = K.images(BOX, kappa, S, theta, phi, NX, NY, anchor, sides,
                   background=bg)
    assert np.array_equal(I_end.T.reshape(3, NX, NY), img)
    geometry = L.probe(BOX, theta, phi, xy, 40)
    assert np.array_equal(rows[:, :3 + 80], geometry, equal_nan=True)
    assert steps.max() <= 40 and steps.max() == K.longest_ray


# ------------------------------------------------- the free-free formulas --

def test_altenhoff_lattice():
    """tau within 8 % of 8.235e-2 T^-1.35 nu_GHz^-2.1 EM (EM in pc cm^-6)"""
    pc = 3.0856775814913673e16
    n = 1.e8            # 100 cm^-3
    depth = 1. * pc
    EM = 100. ** 2 * 1.
    worst = 0.
    for T in (5e3, 8e3, 1e4, 1.5e4):
        for nu in (1e8, 1e9, 5e9, 1e10):
            kappa, _ = K.free_free([n], [T], [0.], [1.], 0.1, [nu])
            tau = kappa[0, 0] * depth
            want = 8.235e-2 * T ** -1.35 * (nu / 1e9) ** -2.1 * EM
            worst = max(worst, abs(tau / want - 1.))
    print("largest deviation from Altenhoff", worst)
    assert worst <= 0.08


def test_thick_and_thin_limits():
    from cmacionize_amd import engine as E
    T, n, depth = 8000., 1.e9, 3.e16
    nu = np.array([3e7, 1e8, 3e10, 1e11])
    kappa, S = K.free_free([n], [T], [0.], [1.], 0.1, nu)
    tau = kappa[:, 0] * depth
    I = S[:, 0] * -np.expm1(-tau)
    assert tau[1] > 40. and tau[2] < 1e-2
    # thick: T_b -> T in the Rayleigh-Jeans regime (h nu / k T = 6e-7)
    Tb = E.brightness_temperature(I, nu)
    assert abs(Tb[0] / T - 1.) < 1e-6 and abs(Tb[1] / T - 1.) < 1e-5
    # thin: index -0.1 (the Gaunt factor's slope), thick: +2
    index = E.continuum_spectral_index(I, nu)
    assert -0.16 < index[2] < -0.08, index
    assert abs(index[0] - 2.) < 1e-3, index
    # Kirchhoff: kappa S is the emissivity, B_nu the module's
    assert np.allclose(S[:, 0], E.planck_function(nu, T), rtol=4 * EPS)


def test_special_cells_give_exact_zeros():
    n = [0., 1e8, 1e8, 1e8, 1e8]
    T = [1e4, 1e4, 0., -5., 1e4]
    xH = [0., 1., 0., 0., 0.5]
    xHe = [0., 1., 0., 0., 1.]
    with np.errstate(all="raise"):
        kappa, S = K.free_free(n, T, xH, xHe, 0.1, [1e7, 1e9, 1e12])
    assert not kappa[:, :4].any() and not S[:, :4].any()
    assert (kappa[:, 4] > 0.).all() and (S[:, 4] > 0.).all()
    assert np.isfinite(kappa).all() and np.isfinite(S).all()
    # B_nu underflows: 1e16 Hz at 500 K has h nu / k T = 960
    kappa, S = K.free_free([1e8], [500.], [0.], [1.], 0.1, [1e16])
    assert kappa[0, 0] == 0. and S[0, 0] == 0.


# ------------------------------------------------------------ the helpers --

def test_module_functions():
    from cmacionize_amd import engine as E
    nu = np.array([1e8, 1e9, 1e10])
    assert E.planck_function(1e9, 0.) == 0.
    B = E.planck_function(nu, 1e4)
    RJ = 2. * nu ** 2 * K.BOLTZMANN * 1e4 / K.LIGHTSPEED ** 2
    assert np.allclose(B, RJ, rtol=1e-4)
    assert np.allclose(E.brightness_temperature(RJ, nu), 1e4, rtol=1e-14)
    cube = RJ[:, None, None] * np.ones((3, 4, 5))
    assert np.allclose(E.brightness_temperature(cube, nu), 1e4, rtol=1e-14)
    index = E.continuum_spectral_index(cube, nu)
    assert index.shape == (2, 4, 5) and np.allclose(index, 2., atol=1e-12)
    cube[1, 0, 0] = 0.
    assert np.isnan(E.continuum_spectral_index(cube, nu)[:, 0, 0]).all()
    with pytest.raises(ValueError):
        E.continuum_spectral_index(cube, nu[:2])
    flux = E.continuum_flux_density(np.ones((3, 4, 5)), 2e-6)
    assert np.allclose(flux, 20 * 2e-6)
    omega = np.arange(20.).reshape(4, 5)
    assert np.allclose(E.continuum_flux_density(np.ones((3, 4, 5)), omega),
                       omega.sum())


def test_symbols_and_methods():
    from cmacionize_amd import engine as E
    header = open(os.path.join(L.ROOT, "include", "cmi_gpu.h")).read()
    for name in ("cmi_gpu_free_free_coefficients",
                 "cmi_gpu_render_continuum_images",
                 "cmi_gpu_render_field_continuum_images",
                 "cmi_gpu_render_continuum_sky",
                 "cmi_gpu_render_field_continuum_sky",
                 "cmi_gpu_render_continuum_sky_map",
                 "cmi_gpu_continuum_probe"):
        assert name in E.EXPORTED_SYMBOLS
        assert re.search(r"\b%s\(" % name, header)
        assert hasattr(E.load_library(), name)
    for name in ("free_free_coefficients", "render_continuum_images",
                 "render_field_continuum_images", "render_continuum_sky",
                 "render_field_continuum_sky", "render_continuum_sky_map",
                 "continuum_probe"):
        assert callable(getattr(E.GpuEngine, name))


def test_refusals_that_need_no_device():
    """null pointers are refused by the C ABI before anything is touched"""
    from cmacionize_amd import engine as E
    lib = E.load_library()
    out = np.zeros(4)
    assert lib.cmi_gpu_free_free_coefficients(None, 1, K._p(out), K._p(out),
                                              K._p(out)) != 0
    assert b"free_free_coefficients: null argument" in \
        lib.cmi_gpu_last_error()
    assert lib.cmi_gpu_render_field_continuum_sky(
        None, 1, K._p(out), K._p(out), None, K._p(out), 1, K._p(out),
        K._p(out)) != 0
    assert b"render_field_continuum_sky: null argument" in \
        lib.cmi_gpu_last_error()
    assert lib.cmi_gpu_continuum_probe(None, 1, K._p(out), K._p(out), None,
                                       0, K._p(out), 1, K._p(out), 4,
                                       K._p(out)) != 0
    assert b"continuum_probe: bad argument" in lib.cmi_gpu_last_error()


# ------------------------------------------------------------ the driver --

ONE_VIEW = open(os.path.join(GOLDEN, "one_view_lines.param")).read()
USED = open(os.path.join(GOLDEN, "one_view_lines.param.usedvalues")).read()
PLAIN = ("EmissivityValues:\n  Halpha: true\nEmissionImages:\n"
         "  view theta: 60. degrees\n")
PLAIN_SKY = ("EmissivityValues:\n  Halpha: true\nEmissionSkyMaps:\n"
             "  observer position: [1.e16 m, 2.e16 m, -3.e16 m]\n")
KEYS = ("  continuum frequencies: 5\n"
        "  continuum frequency minimum: 100. MHz\n"
        "  continuum frequency maximum: 10. GHz\n")


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
    ("  continuum frequencies: 5\n  continuum frequency minimum: 1. GHz\n",
     "%s:continuum frequency maximum is required with "
     "%s:continuum frequencies"),
    (KEYS.replace("frequencies: 5", "frequencies: 0"),
     "%s:continuum frequencies must be between 1 and 2^20 (0 asked for)"),
    (KEYS.replace("frequencies: 5", "frequencies: 1048577"),
     "%s:continuum frequencies must be between 1 and 2^20 (1048577 asked "
     "for)"),
    (KEYS.replace("maximum: 10. GHz", "maximum: 50. MHz"),
     "%s:continuum frequency maximum must be above continuum frequency "
     "minimum"),
    (KEYS.replace("minimum: 100. MHz", "minimum: -1. Hz"),
     "%s:continuum frequency minimum and maximum must be positive"),
    (KEYS + "  type: PGM\n",
     "%s:continuum frequencies needs type BinaryArray"),
    (KEYS + "  continuum background temperature: -2.7 K\n",
     "%s:continuum background temperature must not be negative"),
])
def test_driver_refuses(tmp_path, block, name, more, message):
    r, _ = _emission(tmp_path, block + more)
    assert r.returncode != 0
    assert message.replace("%s", name) in r.stderr, r.stderr
    assert "Could not open" not in r.stderr


def test_driver_reads_the_keys_only_with_the_switch(tmp_path):
    """with `continuum frequencies` the used-values list the new keys in SI,
    the new units and a wavelength converted; without the switch a file gives
    the used-values it gave before the keys existed, the other new keys are
    not read, and the two blocks are read apart"""
    images = KEYS + "  continuum background temperature: 2.725 K\n"
    sky = ("  continuum frequencies: 1\n"
           "  continuum frequency minimum: 21. cm\n"
           "  continuum frequency maximum: 1420000. kHz\n")
    text = ONE_VIEW.replace("EmissionSkyMaps:\n",
                            images + "EmissionSkyMaps:\n") + sky
    r, used = _emission(tmp_path, text, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    used = open(used).read()
    first, second = used.split("EmissionSkyMaps:")
    for word in ("continuum frequencies: 5",
                 "continuum frequency minimum: 1e+08 Hz # (100. MHz)",
                 "continuum frequency maximum: 1e+10 Hz # (10. GHz)",
                 "continuum background temperature: 2.725 K"):
        assert word in first and word not in second, (word, used)
    wavelength = K.LIGHTSPEED / 0.21
    for word in ("continuum frequencies: 1",
                 "continuum frequency maximum: 1.42e+09 Hz # (1420000. kHz)",
                 "continuum background temperature: 0 K"):
        assert word in second, (word, used)
    got = float(re.search(r"continuum frequency minimum: (\S+) Hz",
                          second).group(1))
    assert abs(got / wavelength - 1.) < 1e-5   # (six digits are printed)
    assert "value not used" not in used
    r, used = _emission(tmp_path, ONE_VIEW, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    assert open(used).read() == USED
    r, used = _emission(
        tmp_path, ONE_VIEW + "  continuum frequency minimum: 1. GHz\n"
        "  continuum background temperature: 3. K\n", dry_run=False)
    text = open(used).read()
    assert "continuum frequency minimum: value not used" in text
    assert "continuum background temperature: value not used" in text


def test_frequency_spacing():
    """the driver's nu_f = nu_min * pow(nu_max / nu_min, f / (N - 1)) in
    numpy: logarithmic, the ends exact to rounding (the GPU driver test
    compares the written file with this)"""
    nu = K.driver_frequencies(5, 1e8, 1e10)
    assert nu[0] == 1e8 and abs(nu[-1] / 1e10 - 1.) < 4 * EPS
    assert np.allclose(nu[1:] / nu[:-1], 10. ** 0.5, rtol=1e-14)
    assert K.driver_frequencies(1, 3e9, 5e9).tolist() == [3e9]


# ------------------------------------------------- the kernels' figures --

# VGPRs and waves per SIMD of the march kernels (gfx950, the Makefile's flags;
# DESIGN.md 4.15 quotes them)
MARCH_FIGURES = {("", 4): (60, 7), ("", 8): (88, 5), ("", 16): (126, 4),
                 ("_sky", 4): (82, 5), ("_sky", 8): (112, 4),
                 ("_sky", 16): (180, 2)}


def test_march_kernels_static_figures():
    """from the kernels' metadata in the compiler's listing (`make asm`,
    made again if a source of the library is newer than it): no march kernel
    of any block width has a private segment (nothing spills, no indexed
    private array), each has the VGPRs stated above, and they fit the stated
    waves per SIMD (512 / waves, in granules of 8)"""
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
        m = name and re.search(r"continuum(_sky)?_march_kernelILi(\d+)E",
                               name.group(1))
        if not m:
            continue
        key = (m.group(1) or "", int(m.group(2)))
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
    # the document quotes the same figures
    design = open(os.path.join(L.ROOT, "DESIGN.md")).read()
    for (kind, fb), (vgprs, waves) in MARCH_FIGURES.items():
        assert "`continuum%s_march_kernel<%d>`: %d VGPRs, %d waves per SIMD" \
            % (kind, fb, vgprs, waves) in design
