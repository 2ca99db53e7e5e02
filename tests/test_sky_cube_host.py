"""Sky cubes without a GPU: the CPU restatement
(tests/support/sky_cube_reference.c) against a numpy transcription of the
contract and against the identities the contract buys, the delta line, the
keys of `cmi-gpu --emission` in the EmissionSkyMaps: block up to the point
where it opens the snapshot, and the march kernel's static figures from the
compiler's listing."""
import os
import re
import subprocess

import numpy as np
import pytest

import scattered_line_lib as SL
import sky_cube_lib as Q
import sky_image_lib as S

# the boxes of test_gpu_sky_image.py
BOX = S.Box((-1., 0.5, 2.), (3., 2., 2.5), (12, 10, 14))
EXACT = S.Box((-1., 0.5, 2.), (3., 1.25, 7.), (12, 10, 14))
INSIDE = BOX.anchor + BOX.sides * np.array([0.43, 0.27, 0.61])
OUTSIDE = BOX.anchor + BOX.sides * np.array([-0.15, 0.4, 1.1])
CSRC = os.path.join(S.ROOT, "cmacionize_amd", "csrc")
LISTING = os.path.join(CSRC, "engine.s")
GOLDEN = os.path.join(S.HERE, "golden", "multi_view")
EPS = np.finfo(np.float64).eps


def random_case(seed, dust, integer_velocities=False):
    rng = np.random.default_rng(seed)
    fields = 10. ** rng.uniform(-2., 1., (2, BOX.n))
    fields[rng.uniform(size=(2, BOX.n)) < 0.1] = 0.
    widths = 10. ** rng.uniform(0., 1.5, (2, BOX.n))
    widths[rng.uniform(size=(2, BOX.n)) < 0.1] = 0.
    if integer_velocities:
        vel = rng.integers(-20, 21, (3, BOX.n)).astype(float)
    else:
        vel = rng.uniform(-20., 20., (3, BOX.n))
    k = 10. ** rng.uniform(-1.5, 0.5, BOX.n) if dust else None
    if dust:
        k[rng.uniform(size=BOX.n) < 0.1] = 0.
    return fields, widths, vel, k


def directions(seed, n, origin):
    rng = np.random.default_rng(seed)
    towards = BOX.anchor + BOX.sides * rng.uniform(0., 1., (n, 3)) - origin
    towards /= np.sqrt((towards * towards).sum(axis=1))[:, None]
    return np.concatenate([S.random_directions(rng, n), towards,
                           S.special_directions()])


@pytest.mark.parametrize("dust", [False, True])
def test_restatement_against_the_numpy_transcription(dust):
    """a handful of rays from inside and from outside, 7 channels that cut
    through the emission, an observer that moves: the C and the numpy
    restatement do the same operations on the same cells, up to the two
    libms' exp, expm1 and erf (rtol 1e-12 of the ray's largest channel)"""
    fields, widths, vel, k = random_case(3, dust)
    v_obs = np.array([3., -7., 5.])
    for origin in (INSIDE, OUTSIDE):
        d = directions(5, 6, origin)[[0, 1, 2, 6, 7, 8, 12, 20, 37]]
        got = Q.render(BOX, fields, widths, origin, d, 7, -30., 25.,
                       extinction=k, velocity=vel, observer_velocity=v_obs)
        want = Q.transcription(BOX, fields, widths, origin, d, 7, -30., 25.,
                               extinction=k, velocity=vel,
                               observer_velocity=v_obs)
        assert got.shape == want.shape == (2, 7, len(d))
        assert (want.sum(axis=1) > 0.).sum() >= 8
        scale = want.max(axis=1, keepdims=True)
        assert (np.abs(got - want) <= 1e-12 * scale).all()
        # not the sky value: the range cuts
        total = S.render(BOX, fields, origin, d, extinction=k)
        assert want.sum() < 0.98 * total.sum()


@pytest.mark.parametrize("dust", [False, True])
def test_identity_1_one_wide_channel_is_the_sky(dust):
    fields, widths, vel, k = random_case(7, dust)
    for origin in (INSIDE, OUTSIDE):
        d = directions(9, 300, origin)
        cube = Q.render(BOX, fields, widths, origin, d, 1, -1000., 1000.,
                        extinction=k, velocity=vel,
                        observer_velocity=(4., 5., -6.))
        sky = S.render(BOX, fields, origin, d, extinction=k)
        assert (sky > 0.).sum() > 0.3 * sky.size
        assert np.array_equal(cube[:, 0], sky)


def test_identity_2_one_vector_added_to_everything_changes_nothing():
    """integer velocities: every v - v_obs is exact, so (v, v_obs), (v -
    v_obs, 0) and (v + a, v_obs + a) are the same call"""
    fields, widths, vel, k = random_case(11, True, integer_velocities=True)
    d = directions(13, 200, INSIDE)
    v_obs = np.array([7., -3., 11.])
    a = np.array([-40., 25., 1000.])
    args = (BOX, fields, widths, INSIDE, d, 12, -35., 37.)
    first = Q.render(*args, extinction=k, velocity=vel,
                     observer_velocity=v_obs)
    assert (first > 0.).sum() > 0.3 * first.size
    assert np.array_equal(first, Q.render(
        *args, extinction=k, velocity=vel - v_obs[:, None]))
    assert np.array_equal(first, Q.render(
        *args, extinction=k, velocity=vel + a[:, None],
        observer_velocity=v_obs + a))
    # and the observer's velocity matters
    assert not np.array_equal(first, Q.render(*args, extinction=k,
                                              velocity=vel))


@pytest.mark.parametrize("dust", [False, True])
def test_identity_3_the_channels_sum_to_the_sky(dust):
    """a covering range: the sum over nchan channels is the sky value within
    (nchan + 8 steps) eps relative - per step the fractions sum to 1 within
    nchan roundings and exp / expm1 are the same calls on both sides -; a
    narrower range gives less, never more"""
    fields, widths, vel, k = random_case(17, dust)
    d = directions(19, 300, INSIDE)
    nchan = 19
    steps = int(S.probe(BOX, INSIDE, d, 0)[:, 2].max())
    reach = np.abs(vel).sum(axis=0).max() + 6. * widths.max()
    sky = S.render(BOX, fields, INSIDE, d, extinction=k)
    cube = Q.render(BOX, fields, widths, INSIDE, d, nchan, -reach, reach,
                    extinction=k, velocity=vel)
    total = cube.sum(axis=1)
    assert (sky > 0.).all()
    tol = (nchan + 8 * steps) * EPS
    assert (np.abs(total - sky) <= tol * sky).all()
    part = Q.render(BOX, fields, widths, INSIDE, d, nchan, 0.02 * reach,
                    0.3 * reach, extinction=k, velocity=vel).sum(axis=1)
    assert (part <= sky * (1. + tol)).all()
    assert part.sum() < 0.75 * sky.sum()


def test_cold_cell_is_a_delta_line_on_the_lower_edge():
    """b == 0 and a uniform velocity along +z, rays along +z and -z from
    inside (d = (0, 0, +-1) exactly, u = +-v_z): a line exactly on a channel
    edge goes to the upper channel, one off the edges to the channel that
    contains it; nothing is NaN, with dust neither"""
    j = np.full(BOX.n, 1.5)
    d = np.array([[0., 0., 1.], [0., 0., -1.]])
    sky = S.render(BOX, j, INSIDE, d)[0]
    vel = np.zeros((3, BOX.n))
    # edges -4, -2, 0, 2, 4, 6
    for vz, up, down in ((2., 3, 1), (2.5, 3, 0), (0., 2, 2), (-4., 0, 4),
                         (5.999, 4, None), (-3.5, 0, 3)):
        vel[2] = vz
        cube = Q.render(BOX, j, np.zeros(BOX.n), INSIDE, d, 5, -4., 6.,
                        velocity=vel)[0]
        assert not np.isnan(cube).any()
        for ray, channel in ((0, up), (1, down)):
            if channel is None:   # u = -5.999 is below vmin
                assert not cube[:, ray].any()
                continue
            assert cube[channel, ray] == sky[ray] > 0., (vz, ray)
            assert not np.delete(cube[:, ray], channel).any()
    vel[2] = 6.   # u = 6 is vmax itself: outside [vmin, vmax)
    cube = Q.render(BOX, j, np.zeros(BOX.n), INSIDE, d, 5, -4., 6.,
                    velocity=vel)[0]
    assert not cube[:, 0].any() and not cube[:, 1].any()
    # the observer moving with the matter sees it at rest: channel 2
    cube = Q.render(BOX, j, np.zeros(BOX.n), INSIDE, d, 5, -4., 6.,
                    velocity=vel, observer_velocity=(0., 0., 6.),
                    extinction=np.full(BOX.n, 0.8))[0]
    assert not np.isnan(cube).any()
    assert (cube[2] > 0.).all() and not np.delete(cube, 2, axis=0).any()


def test_symbols_and_methods():
    from cmacionize_amd import engine as E
    header = open(os.path.join(S.ROOT, "include", "cmi_gpu.h")).read()
    for name in ("cmi_gpu_render_field_sky_cube",
                 "cmi_gpu_render_line_sky_cube",
                 "cmi_gpu_render_line_sky_map_cube"):
        assert name in E.EXPORTED_SYMBOLS
        assert re.search(r"\b%s\(" % name, header)
        assert hasattr(E.load_library(), name)
    for name in ("render_field_sky_cube", "render_line_sky_cube",
                 "render_line_sky_map_cube"):
        assert callable(getattr(E.GpuEngine, name))


# ------------------------------------------------------------ the driver --

ONE_VIEW = open(os.path.join(GOLDEN, "one_view_lines.param")).read()
USED = open(os.path.join(GOLDEN, "one_view_lines.param.usedvalues")).read()
# the golden file without its scattered light: PGM cannot hold Stokes maps
# either, and the refusal under test is the cubes'
PLAIN_SKY = ("EmissivityValues:\n  Halpha: true\nEmissionSkyMaps:\n"
             "  observer position: [1.e16 m, 2.e16 m, -3.e16 m]\n")
CHANNELS = ("  velocity channels: 8\n  velocity minimum: -40. km s^-1\n"
            "  velocity maximum: 40. km s^-1\n")


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


@pytest.mark.parametrize("more, message", [
    ("  velocity channels: 8\n  velocity minimum: -40. km s^-1\n",
     "EmissionSkyMaps:velocity maximum is required with "
     "EmissionSkyMaps:velocity channels"),
    (CHANNELS.replace("maximum: 40.", "maximum: -40."),
     "EmissionSkyMaps:velocity maximum must be above velocity minimum"),
    (CHANNELS.replace("channels: 8", "channels: 0"),
     "EmissionSkyMaps:velocity channels must be at least 1"),
    (CHANNELS + "  velocity field type: Keplerian\n",
     "Unknown EmissionSkyMaps:velocity field type \"Keplerian\""),
    (CHANNELS + "  type: PGM\n",
     "EmissionSkyMaps:velocity channels needs type BinaryArray"),
    (CHANNELS + "  velocity field type: RadialExpansion\n"
     "  expansion velocity: 20. km s^-1\n",
     "EmissionSkyMaps:expansion radius is required for RadialExpansion"),
    (CHANNELS + "  observer velocity: [1. km s^-1, nan km s^-1, 0. km s^-1]\n",
     "EmissionSkyMaps:observer velocity must be finite"),
])
def test_driver_refuses(tmp_path, more, message):
    r, _ = _emission(tmp_path, PLAIN_SKY + more)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert "Could not open" not in r.stderr


def test_driver_reads_the_keys_only_with_channels(tmp_path):
    """with `velocity channels` in the EmissionSkyMaps: block the used-values
    list the new keys, `observer velocity 1` among them; without it a file
    gives the used-values it gave before the keys existed, and the other new
    keys are not read"""
    more = CHANNELS + ("  turbulent velocity dispersion: 2. km s^-1\n"
                       "  velocity field type: RadialExpansion\n"
                       "  expansion velocity: 20. km s^-1\n"
                       "  expansion radius: 1.e17 m\n"
                       "  expansion centre: [1.e16 m, 2.e16 m, -3.e16 m]\n"
                       "  number of observers: 3\n"
                       "  observer position 1: [0. m, 0. m, 0. m]\n"
                       "  exclusion radius 1: 1.e16 m\n"
                       "  observer position 2: [0. m, 1.e16 m, 0. m]\n"
                       "  exclusion radius 2: 1.e16 m\n"
                       "  observer velocity: [1. km s^-1, 0. km s^-1, "
                       "0. km s^-1]\n"
                       "  observer velocity 1: [0. km s^-1, 0. km s^-1, "
                       "-9. km s^-1]\n")
    r, used = _emission(tmp_path, ONE_VIEW + more, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    used = open(used).read()
    new = ("velocity channels: 8", "velocity minimum: -40000 m s^-1",
           "velocity maximum: 40000 m s^-1",
           "turbulent velocity dispersion: 2000 m s^-1",
           "velocity field type: RadialExpansion",
           "expansion velocity: 20000 m s^-1", "expansion radius: 1e+17 m",
           "expansion centre: [1e+16 m, 2e+16 m, -3e+16 m]",
           "observer velocity: [1000 m s^-1, 0 m s^-1, 0 m s^-1]",
           "observer velocity 1: [0 m s^-1, 0 m s^-1, -9000 m s^-1]")
    for word in new:
        assert word in used, (word, used)
    assert "value not used" not in used
    # observer 2 takes observer 0's velocity: its key is not read
    assert "observer velocity 2" not in used
    r, used = _emission(tmp_path, ONE_VIEW, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    assert open(used).read() == USED
    r, used = _emission(
        tmp_path, ONE_VIEW + "  velocity minimum: -40. km s^-1\n"
        "  observer velocity: [1. km s^-1, 0. km s^-1, 0. km s^-1]\n",
        dry_run=False)
    text = open(used).read()
    assert "velocity minimum: value not used" in text
    assert "observer velocity: value not used" in text
    # the cube keys of the two blocks are read apart
    r, used = _emission(
        tmp_path, ONE_VIEW.replace(
            "EmissionSkyMaps:\n", CHANNELS + "EmissionSkyMaps:\n"),
        dry_run=False)
    text = open(used).read()
    sky = text[text.index("EmissionSkyMaps:"):]
    assert "velocity channels" in text and "velocity channels" not in sky


# ------------------------------------------------- the kernel's figures --

def test_march_kernel_static_figures():
    """from the kernel's metadata in the compiler's listing (`make asm`): no
    private segment (nothing spills, no indexed private array) and at most
    the VGPRs that the waves per SIMD of DESIGN.md 4.13 allow: 512 / waves,
    in the allocation's granules of 8"""
    waves = int(re.search(
        r"sky_cube_march_kernel[^\n]*: (\d+) waves per SIMD",
        open(os.path.join(S.ROOT, "DESIGN.md")).read()).group(1))
    limit = 512 // waves // 8 * 8
    if not os.path.exists(LISTING):
        subprocess.run(["make", "-C", CSRC, "asm"], check=True)
    text = open(LISTING).read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = 0
    for entry in re.split(r"\n  - ", meta):
        name = re.search(r"\.name:\s+(\S+)", entry)
        if not name or "sky_cube_march_kernel" not in name.group(1):
            continue
        found += 1
        private = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)",
                                entry).group(1))
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1))
        print(name.group(1), "private segment", private, "VGPRs", vgprs,
              "allowed", limit)
        assert private == 0
        assert vgprs <= limit
    assert found == 1
