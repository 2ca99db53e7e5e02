"""Sky maps on the device (cmi_gpu_render_line_sky, cmi_gpu_render_field_sky,
cmi_gpu_sky_probe, cmi_gpu_render_line_sky_map) against the CPU restatement
(tests/support/sky_image_reference.c, checked on its own in
test_sky_image_host.py) and against themselves."""
import ctypes as C

import numpy as np
import pytest

import sky_image_lib as S
from test_gpu_emissivity import random_state
from test_gpu_line_image import (DUST_SIGMA, FILE_NAMES, LEX_LINES,
                                 lexington_box, plain_engine)
from test_gpu_physics import lexington_engine

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
EINVAL, ESTATE = 1, 3  # include/cmi_gpu.h
# unequal cell sides (0.25, 0.2, 0.17857...), anchor away from the origin
BOX = S.Box((-1., 0.5, 2.), (3., 2., 2.5), (12, 10, 14))
# the same grid with cell sides 0.25, 0.125, 0.5: every wall is a double
EXACT = S.Box((-1., 0.5, 2.), (3., 1.25, 7.), (12, 10, 14))
NMAX = int(BOX.ncell.sum()) + 3


def wall(box, axis, i):
    """wall i of an axis as the march computes it"""
    return box.anchor[axis] + box.cellside[axis] * i


def probe_origins(box):
    a, s, c = box.anchor, box.sides, box.cellside
    inside = a + s * np.array([0.43, 0.27, 0.61])
    on_wall, on_edge = inside.copy(), inside.copy()
    on_wall[0] = wall(box, 0, 5)
    on_edge[0], on_edge[1] = wall(box, 0, 5), wall(box, 1, 4)
    on_corner = np.array([wall(box, 0, 5), wall(box, 1, 4), wall(box, 2, 9)])
    lower_face, upper_face = inside.copy(), inside.copy()
    lower_face[1] = a[1]
    upper_face[2] = a[2] + s[2]
    return {"inside": inside, "wall": on_wall, "edge": on_edge,
            "corner": on_corner, "lower face": lower_face,
            "upper face": upper_face,
            "outside": a + s * np.array([-0.15, 0.4, 1.1]),
            "far outside": a + s * np.array([40., -25., 30.])}


def probe_directions(box, origin, rng):
    """~2000 random directions - half of them towards random points of the
    box, so that an origin far away has rays that hit - and the 26 with zero
    components and ties"""
    towards = box.anchor + box.sides * rng.uniform(0., 1., (1000, 3)) - origin
    towards = towards[(towards * towards).sum(axis=1) > 1e-6]
    towards /= np.sqrt((towards * towards).sum(axis=1))[:, None]
    return np.concatenate([S.random_directions(rng, 1000), towards,
                           S.special_directions()])


@pytest.mark.parametrize("box", [BOX, EXACT], ids=["box", "exact"])
def test_probe_is_the_restatement_ray_for_ray(box):
    """Case 1: t_start, t_out, step counts, cells and path lengths - equal,
    not close: the device does the restatement's IEEE operations."""
    eng = plain_engine(box)
    rng = np.random.default_rng(3)
    zero_steps = 0
    for name, origin in probe_origins(box).items():
        d = probe_directions(box, origin, rng)
        got = eng.sky_probe(origin, d, NMAX)
        want = S.probe(box, origin, d, NMAX)
        steps = want[:, 2].astype(int)
        hit = steps > 0
        first_ds = want[hit, 3 + NMAX]
        zero_steps += int((first_ds == 0.).sum())
        print(name, "rays", len(d), "misses", int((~hit).sum()), "longest",
              steps.max(), "zero-length first steps",
              int((first_ds == 0.).sum()))
        assert hit.sum() > 400 and steps.max() <= NMAX - 3
        if name in ("outside", "far outside", "lower face", "upper face"):
            assert (~hit).sum() > 400
        else:
            assert hit.all()
        assert np.array_equal(got[:, 2], want[:, 2])
        assert np.array_equal(got[:, 3:3 + NMAX], want[:, 3:3 + NMAX])
        assert np.array_equal(got[:, 3 + NMAX:], want[:, 3 + NMAX:])
        assert np.array_equal(got[:, :2], want[:, :2], equal_nan=True)
    if box is EXACT:
        # wall, edge and corner: every ray pointing back across a wall
        assert zero_steps > 2000
    eng.close()


def sky_cases(box, rng):
    """(origin, directions): inside with 1000 rays (the last wave partial),
    outside, and a single ray"""
    o = probe_origins(box)
    return [(o["inside"], probe_directions(box, o["inside"], rng)[:1000]),
            (o["corner"], probe_directions(box, o["corner"], rng)),
            (o["outside"], probe_directions(box, o["outside"], rng)),
            (o["inside"], S.random_directions(rng, 1))]


@pytest.mark.parametrize("nfields", [3, 9])
def test_field_skies_match_the_restatement(nfields):
    """Cases 2 and 3: random positive fields, one and two batches. Without
    extinction equal bit for bit (the same terms in the same order, T = 1).
    With random extinction within 8 eps (steps + 1) of the longest ray: per
    step one exp, one expm1 (at most 2 ulp in either libm), three
    multiplications and an addition, (3 n + 6) eps over both sides."""
    eng = plain_engine(BOX)
    rng = np.random.default_rng(17 + nfields)
    fields = 10. ** rng.uniform(-2., 1., (nfields, BOX.n))
    # optical depths per cell around 0.1, some cells without dust
    k = 10. ** rng.uniform(-1.5, 0.5, BOX.n)
    k[rng.uniform(size=BOX.n) < 0.1] = 0.
    for origin, d in sky_cases(BOX, rng):
        want = S.render(BOX, fields, origin, d)
        got = eng.render_field_sky(fields, origin, d)
        assert got.shape == want.shape == (nfields, len(d))
        assert (want > 0.).sum() > 0.3 * want.size
        assert np.array_equal(got, want)
        nsteps = int(S.probe(BOX, origin, d, 0)[:, 2].max())
        rtol = 8. * EPS * (nsteps + 1)
        want = S.render(BOX, fields, origin, d, extinction=k)
        got = eng.render_field_sky(fields, origin, d, extinction=k)
        err = np.abs(got - want) / np.maximum(want, 1e-300)
        print("rays", len(d), "longest ray", nsteps, "rtol", rtol, "worst",
              err[want > 0.].max())
        assert np.array_equal(got == 0., want == 0.)
        assert (err[want > 0.] <= rtol).all()
    eng.close()


def test_more_rays_than_one_launch_takes():
    """Case 2, last: 2^22 + 1000 rays on the small grid cross the chunking of
    a call: equal to the restatement bit for bit, every ray in its place"""
    eng = plain_engine(BOX)
    rng = np.random.default_rng(5)
    n = (1 << 22) + 1000
    origin = probe_origins(BOX)["inside"]
    d = S.random_directions(rng, n)
    field = 10. ** rng.uniform(-2., 1., BOX.n)
    want = S.render(BOX, field, origin, d)
    got = eng.render_field_sky(field, origin, d)
    assert got.shape == (1, n) and (want > 0.).all()
    assert np.array_equal(got, want)
    eng.close()


def test_line_skies_end_to_end(oracle):
    """Case 4: the random lexington state of test_line_images_end_to_end:
    device emissivities, records and march against the restatement fed with
    the oracle's emissivities, at that test's rtol 2e-10 (1e-10 for an
    emissivity, carried through a sum of positive terms, plus the march's own
    bound). From inside and from outside, without and with dust."""
    from cmacionize_amd import engine as E
    import oracle_lib as o
    ncell = 12
    sim = oracle.lexington_simulation(ncell)
    density, temperature, x = random_state(ncell, 7)
    eng = lexington_engine(ncell)
    eng.upload_cells(density, temperature, x)
    box = lexington_box(ncell)
    n = ncell ** 3
    ref = np.array([oracle.emissivities(sim.model, density[c], temperature[c],
                                        x[:, c]) for c in range(n)]).T
    idx = [E.EMISSION_LINES.index(name) for name in LEX_LINES]
    rng = np.random.default_rng(11)
    for origin in (np.array([1., -0.5, 0.3]) * o.PC,
                   np.array([-7., 2., 6.]) * o.PC):
        d = probe_directions(box, origin, rng)[700:2000]
        for sigma in (0., DUST_SIGMA):
            got = eng.render_line_sky(LEX_LINES, origin, d, sigma)
            assert list(got) == LEX_LINES
            want = S.render(box, ref[idx], origin, d,
                            extinction=density * sigma if sigma else None)
            for k, name in enumerate(LEX_LINES):
                assert got[name].shape == (len(d),)
                lit = want[k] > 0.
                assert lit.sum() > 0.3 * len(d)
                assert not got[name][~lit].any(), name
                err = np.abs(got[name] - want[k])[lit] / want[k][lit]
                print(name, "sigma", sigma, "worst", err.max())
                assert err.max() < 2.e-10, (name, sigma, err.max())
            if sigma:
                plain = eng.render_line_sky(["HAlpha"], origin, d)["HAlpha"]
                assert (got["HAlpha"] <= plain).all()
                assert got["HAlpha"].sum() < plain.sum()
    eng.close()


def test_map_is_the_ray_list_in_any_order():
    """Case 5: the map call marches its rays in 8 x 8 tiles; its pixels are
    those of the ray-list call on sky_map_directions' rays, bit for bit (37
    and 21 are no multiples of 8), full sky and a window in a turned frame;
    a second call gives the same bits."""
    from cmacionize_amd import engine as E
    import oracle_lib as o
    ncell = 10
    density, temperature, x = random_state(ncell, 23)
    eng = lexington_engine(ncell)
    eng.upload_cells(density, temperature, x)
    lines = ["HAlpha", "OIII_5007", "NII_6584"]
    origin = np.array([1., -0.5, 0.3]) * o.PC
    c, s = np.cos(0.4), np.sin(0.4)
    frame = np.array([[c, s, 0.], [0., 0., 1.], [s, -c, 0.]])
    nlon, nlat = 37, 21
    for kw in ({}, dict(lon_range=(0.2, 1.7), lat_range=(-0.3, 0.9),
                        frame=frame)):
        d, omega = E.sky_map_directions(nlon, nlat, **kw)
        rays = eng.render_line_sky(lines, origin, d, DUST_SIGMA)
        maps = eng.render_line_sky_map(lines, origin, nlon, nlat,
                                       dust_cross_section=DUST_SIGMA, **kw)
        again = eng.render_line_sky_map(lines, origin, nlon, nlat,
                                        dust_cross_section=DUST_SIGMA, **kw)
        for name in lines:
            assert maps[name].shape == (nlon, nlat)
            assert (maps[name] > 0.).mean() > 0.9
            assert np.array_equal(maps[name].reshape(-1), rays[name]), name
            assert np.array_equal(maps[name], again[name]), name
        # the map's columns differ (it is no constant) and a flux exists
        assert maps["HAlpha"].std() > 0.
        assert (maps["HAlpha"].reshape(-1) * omega).sum() > 0.
    eng.close()


def test_bad_arguments_are_refused_and_the_engine_lives():
    """Case 6: every refusal of the contract returns its code, and after each
    a valid call still works"""
    from cmacionize_amd import GpuEngine
    from cmacionize_amd import engine as E
    lib = E.load_library()
    eng = lexington_engine(4)
    out = (C.c_double * 64)()
    line = (C.c_int32 * 2)(0, 1)
    dbl3 = C.c_double * 3
    frame = (C.c_double * 9)(1., 0., 0., 0., 1., 0., 0., 0., 1.)
    field = (C.c_double * 64)(*([1.] * 64))
    half = 0.5 * np.pi

    def lines(nlines=1, origin=(0., 0., 0.), nrays=1, d=(0., 0.6, 0.8),
              sigma=0.):
        return lib.cmi_gpu_render_line_sky(eng._h, nlines, line,
                                           dbl3(*origin), nrays, dbl3(*d),
                                           sigma, out)

    def fields(nfields=1, origin=(0., 0., 0.), nrays=1, d=(0., 0.6, 0.8)):
        return lib.cmi_gpu_render_field_sky(eng._h, nfields, field,
                                            dbl3(*origin), nrays, dbl3(*d),
                                            None, out)

    def probe(origin=(0., 0., 0.), n=1, d=(0., 0.6, 0.8), max_cells=4):
        return lib.cmi_gpu_sky_probe(eng._h, dbl3(*origin), n, dbl3(*d),
                                     max_cells, out)

    def sky_map(origin=(0., 0., 0.), f=frame, lon=(-np.pi, np.pi),
                lat=(-half, half), nlon=4, nlat=4, sigma=0.):
        return lib.cmi_gpu_render_line_sky_map(
            eng._h, 1, line, dbl3(*origin), f, lon[0], lon[1], lat[0],
            lat[1], nlon, nlat, sigma, out)

    assert lines() == ESTATE
    assert b"cell data" in lib.cmi_gpu_last_error()
    assert sky_map() == ESTATE
    eng.upload_cells(np.full(64, 1e8), np.full(64, 8000.),
                     np.full((14, 64), 1e-3))
    nan, inf = float("nan"), float("inf")
    for call in (lines, fields, probe):
        assert call() == 0
        for which in range(3):
            for bad in (nan, inf, -inf):
                v = [0., 0., 0.]
                v[which] = bad
                assert call(origin=v) == EINVAL
                assert b"origin" in lib.cmi_gpu_last_error()
                v = [0., 0.6, 0.8]
                v[which] = bad
                assert call(d=v) == EINVAL
                assert b"not finite" in lib.cmi_gpu_last_error()
            assert call() == 0
        # |d|^2 = 1 +- 3e-9 is refused, 1 +- 5e-10 is not
        for scale, rc in ((1. + 1.5e-9, EINVAL), (1. - 1.5e-9, EINVAL),
                          (1. + 2.5e-10, 0), (1. - 2.5e-10, 0),
                          (0., EINVAL), (2., EINVAL)):
            assert call(d=(0., 0.6 * scale, 0.8 * scale)) == rc, scale
            if rc:
                assert b"unit vector" in lib.cmi_gpu_last_error()
        assert call(d=(0., 0., -1.)) == 0  # zero components are allowed
        assert call() == 0
    assert lines(nrays=0) == EINVAL and lines(nrays=-1) == EINVAL
    assert lines(nrays=(1 << 28) + 1) == EINVAL
    assert b"rays" in lib.cmi_gpu_last_error()
    assert fields(nrays=0) == EINVAL and fields(nrays=(1 << 28) + 1) == EINVAL
    assert probe(n=0) == EINVAL and probe(n=(1 << 24) + 1) == EINVAL
    assert probe(max_cells=-1) == EINVAL
    assert lines(sigma=-1.e-30) == EINVAL and lines(sigma=nan) == EINVAL
    assert b"cross section" in lib.cmi_gpu_last_error()
    assert lines(nlines=0) == EINVAL and lines(nlines=43) == EINVAL
    line[1] = 42
    assert lines(nlines=2) == EINVAL
    assert b"no emission line 42" in lib.cmi_gpu_last_error()
    line[1] = 1
    assert lines(nlines=2) == 0
    assert fields(nfields=0) == EINVAL and fields() == 0
    # the map call
    assert sky_map() == 0
    tilted = (C.c_double * 9)(1., 0., 0., 0., 1., 0., 0., 1e-6, 1.)
    longer = (C.c_double * 9)(1. + 1e-8, 0., 0., 0., 1., 0., 0., 0., 1.)
    assert sky_map(f=tilted) == EINVAL and sky_map(f=longer) == EINVAL
    assert b"orthonormal" in lib.cmi_gpu_last_error()
    assert sky_map(nlon=0) == EINVAL and sky_map(nlat=-2) == EINVAL
    assert sky_map(nlon=1 << 15, nlat=(1 << 13) + 1) == EINVAL
    assert sky_map(lon=(1., 1.)) == EINVAL and sky_map(lon=(0., inf)) == EINVAL
    assert sky_map(lat=(-2., 1.)) == EINVAL and sky_map(lat=(0.3, 0.1)) == EINVAL
    assert sky_map(origin=(0., nan, 0.)) == EINVAL
    assert sky_map(sigma=-1.) == EINVAL
    assert sky_map() == 0
    # a missed ray in the probe: no steps, NaN
    row = eng.sky_probe((1e30, 0., 0.), [[1., 0., 0.]], 4)[0]
    assert row[2] == 0. and np.isnan(row[:2]).all() and not row[3:].any()
    # the engine still computes
    assert eng.compute_emissivities(["HAlpha"])["HAlpha"].min() > 0.
    eng.close()

    d = [[0., 0.6, 0.8]]
    periodic = GpuEngine((4, 4, 4), (0., 0., 0.), (1., 1., 1.), (1, 0, 0),
                         device=0)
    with pytest.raises(E.EngineError, match="periodic"):
        periodic.render_field_sky(np.ones(64), (0.5, 0.5, 0.5), d)
    with pytest.raises(E.EngineError, match="periodic"):
        periodic.sky_probe((0.5, 0.5, 0.5), d, 4)
    periodic.close()
    block = GpuEngine((8, 4, 4), (0., 0., 0.), (1., 1., 1.), (0, 0, 0),
                      device=0, sub_offset=(4, 0, 0), sub_ncell=(4, 4, 4))
    with pytest.raises(E.EngineError, match="decomposed"):
        block.render_field_sky(np.ones(64), (0.5, 0.5, 0.5), d)
    with pytest.raises(E.EngineError, match="decomposed"):
        block.sky_probe((0.5, 0.5, 0.5), d, 4)
    assert block.n == 64
    block.close()


def test_driver_writes_the_sky_maps_of_a_snapshot(tmp_path):
    """Case 7: `cmi-gpu --emission` with an EmissionSkyMaps block on the
    snapshot of a short lexington run: each .dat is render_line_sky_map of
    the same state with the frame the block describes, equal; the snapshot
    gets the datasets it gets without the block."""
    import os
    import shutil
    import subprocess
    import hdf5_mini
    import oracle_lib as o
    root = S.ROOT
    exe = os.path.join(root, "cmacionize_amd", "cmi-gpu")
    bench = os.path.join(root, "benchmarks")
    ncell = 14
    text = open(os.path.join(bench, "lexingtonHII40.param")).read()
    text = text.replace("[64, 64, 64]", "[%d, %d, %d]" % ((ncell,) * 3))
    text = text.replace("number of photons: 1e8", "number of photons: 30000")
    text = text.replace("number of iterations: 20", "number of iterations: 6")
    text = text.replace("NumberDensity: 0", "NumberDensity: 1")
    shutil.copy(os.path.join(bench, "lexingtonHII40.yml"), tmp_path)
    (tmp_path / "run.param").write_text(text)
    r = subprocess.run([exe, "--params", "run.param"], capture_output=True,
                       text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    snapshot = str(tmp_path / "lexingtonHII40_006.hdf5")
    plain = str(tmp_path / "plain.hdf5")
    shutil.copy(snapshot, plain)

    nlon, nlat, sigma = 40, 22, 2.e-27
    observer = (5.e16, -3.e16, 2.e16)
    lon, lat = (-1., 2.), (-0.5, 1.)
    pole, zero = (0., 0., 2.), (0., 3., 1.)
    switches = "EmissivityValues:\n" + "".join(
        "  %s: true\n" % name for name in FILE_NAMES)
    block = ("EmissionSkyMaps:\n"
             "  observer position: [%r m, %r m, %r m]\n"
             "  number of longitude pixels: %d\n"
             "  number of latitude pixels: %d\n"
             "  longitude range: [%r radians, %r radians]\n"
             "  latitude range: [%r radians, %r radians]\n"
             "  frame pole: [%r, %r, %r]\n"
             "  frame zero longitude: [%r, %r, %r]\n"
             "  dust cross section per hydrogen: %r m^2\n"
             "  filename prefix: sky\n  output folder: %s\n" %
             (observer + (nlon, nlat) + lon + lat + pole + zero +
              (sigma, str(tmp_path))))
    (tmp_path / "sky.param").write_text(switches + block)
    (tmp_path / "lines.param").write_text(switches)
    r = subprocess.run([exe, "--emission", "--params", "sky.param", "--file",
                        snapshot], capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "--emission", "--params", "lines.param",
                        "--file", plain], capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert not [n for n in os.listdir(tmp_path)
                if n.startswith("sky_map") or n.startswith("line_image")]
    with_maps, without = hdf5_mini.read(snapshot), hdf5_mini.read(plain)
    assert sorted(with_maps["/PartType0"].members) == \
        sorted(without["/PartType0"].members)
    for name, node in without["/PartType0"].members.items():
        assert np.array_equal(with_maps["/PartType0/" + name].data,
                              node.data), name
    used = open(str(tmp_path / "sky.param.used-values")).read()
    assert "EmissionSkyMaps:" in used and "type: BinaryArray" in used
    assert "EmissionSkyMaps" not in \
        open(str(tmp_path / "lines.param.used-values")).read()

    # the same state on an engine of our own, every cell where its
    # coordinates put it
    f = without
    ions = ["H", "He", "C+", "C++", "N", "N+", "N++", "O", "O+", "Ne", "Ne+",
            "S+", "S++", "S+++"]
    unit_length = 0.01 * float(np.ravel(
        f["/Units"].attrs["Unit length in cgs (U_L)"])[0])
    box_sides = 10. * o.PC
    mid = f["/PartType0/Coordinates"].data.reshape(-1, 3) * unit_length
    idx = np.floor(ncell * mid / box_sides).astype(np.int64)
    cell = (idx[:, 0] * ncell + idx[:, 1]) * ncell + idx[:, 2]
    assert sorted(cell) == list(range(ncell ** 3))

    def placed(values):
        out = np.empty_like(values)
        out[..., cell] = values
        return out

    unit_n = 1. / unit_length ** 3
    eng = lexington_engine(ncell)
    eng.upload_cells(
        placed(f["/PartType0/NumberDensity"].data * unit_n),
        placed(f["/PartType0/Temperature"].data * float(np.ravel(
            f["/Units"].attrs["Unit temperature in cgs (U_T)"])[0])),
        placed(np.array([f["/PartType0/NeutralFraction" + i].data
                         for i in ions])))
    # the driver's Gram-Schmidt: the pole is kept, the zero of longitude made
    # perpendicular to it, the third axis is pole x zero longitude (exact for
    # these vectors)
    frame = [[0., 1., 0.], [-1., 0., 0.], [0., 0., 1.]]
    want = eng.render_line_sky_map(list(FILE_NAMES.values()), observer, nlon,
                                   nlat, lon, lat, frame, sigma)
    for file_name, name in FILE_NAMES.items():
        got = np.fromfile(str(tmp_path / ("sky_%s.dat" % file_name)))
        assert got.shape == (nlon * nlat,)
        assert got.max() > 0.
        assert np.array_equal(got.reshape(nlon, nlat), want[name]), name
    eng.close()
