"""Spectral line cubes without a GPU: the CPU restatement
(tests/support/line_cube_reference.c) against numpy and against the identities
the contract buys, the Python helpers, the exported symbols, the keys of
`cmi-gpu --emission` up to the point where it opens the snapshot, and the
march kernel's static figures from the compiler's listing."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import line_cube_lib as Q
import line_image_lib as L
import scattered_line_lib as S

BOX, NX, NY, VIEWS = Q.BOX, Q.NX, Q.NY, Q.VIEWS
CSRC = os.path.join(L.ROOT, "cmacionize_amd", "csrc")
LISTING = os.path.join(CSRC, "engine.s")
GOLDEN = os.path.join(L.HERE, "golden", "multi_view")


def test_single_cell_and_uniform_box_against_numpy():
    """One emitting cell without dust: j chord / 4 pi times the analytic
    channel fractions; a uniform box at rest with uniform b: every pixel's
    spectrum is its chord value times the same fractions. rtol 1e-12."""
    nchan, vmin, vmax, b = 7, -30., 40., 11.
    for theta, phi in VIEWS[:1] + VIEWS[3:4]:
        anchor, sides = Q.image_rectangle(BOX, theta, phi)
        n, _, _ = L.axes(theta, phi)
        # the cell (5, 4, 3), moving with (3, -2, 7)
        cell = (5 * BOX.ncell[1] + 4) * BOX.ncell[2] + 3
        j = np.zeros(BOX.n)
        j[cell] = 2.5
        vel = np.zeros((3, BOX.n))
        vel[:, cell] = (3., -2., 7.)
        u = -float(np.dot(n, (3., -2., 7.)))
        cube = Q.render(BOX, j, np.full(BOX.n, b), theta, phi, NX, NY, anchor,
                        sides, nchan, vmin, vmax, velocity=vel)[0]
        image = L.render(BOX, j, theta, phi, NX, NY, anchor, sides)[0]
        f = Q.fractions(nchan, vmin, vmax, u, b)
        assert image.max() > 0. and 0.5 < f.sum() < 1.
        assert np.allclose(cube, image[None] * f[:, None, None], rtol=1e-12,
                           atol=0.)
        # the image itself is j chord / 4 pi of the one cell
        lo = BOX.anchor + np.array([5, 4, 3]) * BOX.cellside
        one = L.Box(lo, BOX.cellside, (1, 1, 1))
        xy = L.sample_coordinates(NX, NY, anchor, sides).reshape(-1, 2)
        chord = L.chords(one, theta, phi, xy).reshape(NX, NY)
        assert np.allclose(image, 2.5 * chord / (4. * np.pi), rtol=1e-9,
                           atol=1e-12)

        cube = Q.render(BOX, np.full(BOX.n, 0.7), np.full(BOX.n, b), theta,
                        phi, NX, NY, anchor, sides, nchan, vmin, vmax)[0]
        chord = L.chords(BOX, theta, phi, xy).reshape(NX, NY)
        f = Q.fractions(nchan, vmin, vmax, 0., b)
        assert (chord == 0.).sum() > 20
        want = (0.7 * chord / (4. * np.pi))[None] * f[:, None, None]
        assert np.allclose(cube, want, rtol=1e-12, atol=0.)


def random_case(seed, dust):
    rng = np.random.default_rng(seed)
    fields = 10. ** rng.uniform(-2., 1., (2, BOX.n))
    widths = 10. ** rng.uniform(0., 1.5, (2, BOX.n))
    vel = rng.uniform(-20., 20., (3, BOX.n))
    k = 10. ** rng.uniform(-1.5, 0.5, BOX.n) if dust else None
    return fields, widths, vel, k


@pytest.mark.parametrize("dust", [False, True])
def test_identity_1_one_wide_channel_is_the_image(dust):
    fields, widths, vel, k = random_case(5, dust)
    for (theta, phi), s in zip(VIEWS, (1, 2, 1, 2, 1, 2)):
        anchor, sides = Q.image_rectangle(BOX, theta, phi)
        cube = Q.render(BOX, fields, widths, theta, phi, NX, NY, anchor,
                        sides, 1, -1000., 1000., s, extinction=k,
                        velocity=vel)
        image = L.render(BOX, fields, theta, phi, NX, NY, anchor, sides, s,
                         extinction=k)
        assert (image > 0.).sum() > 0.3 * image.size
        assert np.array_equal(cube[:, 0], image)


def test_identity_2_a_shift_of_everything_changes_nothing():
    """theta = 0: n = (0, 0, 1) exactly; velocities, edges and D in multiples
    of 2^-3, so that every e - u is exact"""
    rng = np.random.default_rng(9)
    fields = 10. ** rng.uniform(-2., 1., (1, BOX.n))
    widths = 10. ** rng.uniform(0., 1., (1, BOX.n))
    vel = np.zeros((3, BOX.n))
    vel[2] = rng.integers(-80, 81, BOX.n) / 8.
    k = 10. ** rng.uniform(-1.5, 0.5, BOX.n)
    anchor, sides = Q.image_rectangle(BOX, 0., 0.)
    D = 40.
    a = Q.render(BOX, fields, widths, 0., 0., NX, NY, anchor, sides, 12, -9.,
                 9., extinction=k, velocity=vel)
    shifted = vel.copy()
    shifted[2] -= D   # u = -v_z grows by D
    b = Q.render(BOX, fields, widths, 0., 0., NX, NY, anchor, sides, 12,
                 -9. + D, 9. + D, extinction=k, velocity=shifted)
    assert (a > 0.).sum() > 0.3 * a.size
    assert np.array_equal(a, b)


def test_cold_cell_is_a_delta_line_on_the_lower_edge():
    """b == 0: a line exactly on a channel edge goes to the upper channel,
    one off the edges to the channel that contains it; nothing is NaN"""
    anchor, sides = Q.image_rectangle(BOX, 0., 0.)
    j = np.full(BOX.n, 1.5)
    vel = np.zeros((3, BOX.n))
    image = L.render(BOX, j, 0., 0., NX, NY, anchor, sides)[0]
    for vz, channel in ((-2., 3), (-2.5, 3), (0., 2), (4., 0), (-5.999, 4)):
        vel[2] = vz   # u = -vz; edges -4, -2, 0, 2, 4, 6
        cube = Q.render(BOX, j, np.zeros(BOX.n), 0., 0., NX, NY, anchor,
                        sides, 5, -4., 6., velocity=vel)[0]
        assert not np.isnan(cube).any()
        assert np.array_equal(cube[channel], image), (vz, channel)
        assert not np.delete(cube, channel, axis=0).any()
    for vz in (-6., 4.5):   # u = 6 is vmax itself: outside [vmin, vmax)
        vel[2] = vz
        cube = Q.render(BOX, j, np.zeros(BOX.n), 0., 0., NX, NY, anchor,
                        sides, 5, -4., 6., velocity=vel)[0]
        assert not cube.any()
    # and with dust, where 0 * inf would show
    cube = Q.render(BOX, j, np.zeros(BOX.n), 0., 0., NX, NY, anchor, sides, 5,
                    -4., 6., extinction=np.full(BOX.n, 0.8), velocity=vel)
    assert not np.isnan(cube).any()


def test_cube_moments_of_a_gaussian():
    from cmacionize_amd import engine as E
    nchan, vmin, vmax = 400, -50.e3, 70.e3
    centres = E.cube_channel_centres(nchan, vmin, vmax)
    assert centres.shape == (nchan,)
    assert centres[0] == vmin + 0.5 * (vmax - vmin) / nchan
    u, sigma = 7.e3, 9.e3
    f = Q.fractions(nchan, vmin, vmax, u, math.sqrt(2.) * sigma)
    cube = np.zeros((nchan, 2, 3))
    cube[:, 0, 0] = 4. * f
    cube[:, 1, 2] = f
    m0, mean, disp = E.cube_moments(cube, centres)
    assert m0.shape == mean.shape == disp.shape == (2, 3)
    assert m0[0, 0] == pytest.approx(4., rel=1e-9)
    assert mean[0, 0] == pytest.approx(u, rel=1e-6)
    # a channel of width dv adds dv^2 / 12 to the variance
    dv = (vmax - vmin) / nchan
    assert disp[1, 2] == pytest.approx(math.sqrt(sigma ** 2 + dv ** 2 / 12.),
                                       rel=1e-6)
    dark = np.ones((2, 3), dtype=bool)
    dark[0, 0] = dark[1, 2] = False
    assert not m0[dark].any()
    assert np.isnan(mean[dark]).all() and np.isnan(disp[dark]).all()
    # a leading axis of lines
    m0b, _, _ = E.cube_moments(cube[None], centres)
    assert m0b.shape == (1, 2, 3)


def test_symbols_and_the_table_of_atomic_weights():
    from cmacionize_amd import engine as E
    for name in ("cmi_gpu_set_cell_velocities", "cmi_gpu_render_line_cube",
                 "cmi_gpu_render_field_cube"):
        assert name in E.EXPORTED_SYMBOLS
        assert re.search(r"\b%s\(" % name, open(os.path.join(
            L.ROOT, "include", "cmi_gpu.h")).read())
    for name in ("set_cell_velocities", "render_line_cube",
                 "render_field_cube"):
        assert callable(getattr(E.GpuEngine, name))
    w = E.LINE_ATOMIC_WEIGHTS
    assert len(w) == 31
    assert w["HAlpha"] == w["HBeta"] == 1.00794
    assert w["HeI_5876"] == 4.002602
    assert w["CII_158mu"] == w["CIII_1908"] == 12.0107
    assert w["NII_6584"] == w["NIII_57mu"] == 14.0067
    assert w["OI_6300"] == w["OII_3727"] == w["OIII_88mu"] == 15.9994
    assert w["NeII_12mu"] == w["NeIII_15mu"] == 20.1797
    assert w["SII_6725"] == w["SIV_10mu"] == 32.065
    for name in ("HII", "BALMER_JUMP_LOW", "BALMER_JUMP_HIGH", "avg_T",
                 "avg_T_count", "avg_nH_nHe", "avg_nH_nHe_count", "Hrec_s",
                 "WFC2_F439W", "WFC2_F555W", "WFC2_F675W"):
        assert name not in w
    # the engine's own table, in the order of EMISSION_LINES
    lib = E.load_library()
    assert "cmi_gpu_emission_line_atomic_weight" in E.EXPORTED_SYMBOLS
    values = [lib.cmi_gpu_emission_line_atomic_weight(i)
              for i in range(len(E.EMISSION_LINES))]
    assert values == [w.get(name, 0.) for name in E.EMISSION_LINES]
    assert lib.cmi_gpu_emission_line_atomic_weight(-1) == 0.
    assert lib.cmi_gpu_emission_line_atomic_weight(42) == 0.


# ------------------------------------------------------------ the driver --

ONE_VIEW = open(os.path.join(GOLDEN, "one_view_lines.param")).read()
USED = open(os.path.join(GOLDEN, "one_view_lines.param.usedvalues")).read()
IMAGES, SKY = ONE_VIEW.split("EmissionSkyMaps:\n")
SKY = "EmissionSkyMaps:\n" + SKY
CHANNELS = ("  velocity channels: 8\n  velocity minimum: -40. km s^-1\n"
            "  velocity maximum: 40. km s^-1\n")


def _emission(tmp_path, text, dry_run=True):
    params = tmp_path / "lines.param"
    params.write_text(text)
    used = str(params) + ".used-values"
    if os.path.exists(used):
        os.remove(used)
    cmd = [S.CMI_GPU, "--emission", "--params", str(params), "--file",
           str(tmp_path / "nowhere.hdf5")]
    if dry_run:
        cmd.insert(2, "--dry-run")
    r = subprocess.run(cmd, capture_output=True, text=True,
                       cwd=str(tmp_path))
    return r, used


@pytest.mark.parametrize("more, message", [
    (CHANNELS.replace("maximum: 40.", "maximum: -40."),
     "EmissionImages:velocity maximum must be above velocity minimum"),
    (CHANNELS.replace("maximum: 40.", "maximum: -50."),
     "EmissionImages:velocity maximum must be above velocity minimum"),
    (CHANNELS.replace("channels: 8", "channels: 0"),
     "EmissionImages:velocity channels must be at least 1"),
    (CHANNELS + "  velocity field type: Keplerian\n",
     "Unknown EmissionImages:velocity field type \"Keplerian\""),
    (CHANNELS + "  type: PGM\n",
     "EmissionImages:velocity channels needs type BinaryArray"),
])
def test_driver_refuses(tmp_path, more, message):
    text = IMAGES + more
    r, _ = _emission(tmp_path, text)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert "Could not open" not in r.stderr


def test_driver_reads_the_keys_only_with_channels(tmp_path):
    """with `velocity channels` the used-values list the new keys; without
    it a file gives the used-values it gave before the keys existed, and
    the other new keys are not read"""
    more = CHANNELS + ("  turbulent velocity dispersion: 2. km s^-1\n"
                       "  velocity field type: RadialExpansion\n"
                       "  expansion velocity: 20. km s^-1\n"
                       "  expansion radius: 1.e17 m\n")
    r, used = _emission(tmp_path, IMAGES + more + SKY, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    used = open(used).read()
    new = ("velocity channels: 8", "velocity minimum: -40000 m s^-1",
           "velocity maximum: 40000 m s^-1",
           "turbulent velocity dispersion: 2000 m s^-1",
           "velocity field type: RadialExpansion",
           "expansion velocity: 20000 m s^-1", "expansion radius: 1e+17 m",
           "expansion centre: [0 m, 0 m, 0 m]")
    for word in new:
        assert word in used, (word, used)
    assert "value not used" not in used
    rest = [l for l in used.split("\n")
            if not any(l.strip().startswith(w.split(":")[0]) for w in new)]
    assert rest == USED.split("\n")
    r, used = _emission(tmp_path, ONE_VIEW, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    assert open(used).read() == USED
    r, used = _emission(
        tmp_path, IMAGES + "  velocity minimum: -40. km s^-1\n" + SKY,
        dry_run=False)
    assert "velocity minimum: value not used" in open(used).read()


# ------------------------------------------------- the kernel's figures --

def test_march_kernel_static_figures():
    """from the kernel's metadata in the compiler's listing (`make asm`): no
    private segment (nothing spills, no indexed private array), at most 128
    VGPRs (four waves per SIMD)"""
    if not os.path.exists(LISTING):
        subprocess.run(["make", "-C", CSRC, "asm"], check=True)
    text = open(LISTING).read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = 0
    for entry in re.split(r"\n  - ", meta):
        name = re.search(r"\.name:\s+(\S+)", entry)
        if not name or "line_cube_march_kernel" not in name.group(1):
            continue
        found += 1
        private = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)",
                                entry).group(1))
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1))
        print(name.group(1), "private segment", private, "VGPRs", vgprs)
        assert private == 0
        assert vgprs <= 128
    assert found >= 1
