"""GPU tests of the scattered-light line images: the cell-luminosity source
(cmi_gpu_set_cell_source_line / _field, cmi_gpu_get_cell_source), dust that
follows the gas (cmi_gpu_set_dust_scattering_per_hydrogen), the cell source's
instantiations of the dust kernels, GpuEngine.render_scattered_line_images
and `cmi-gpu --emission` with `scattering: true` - against the CPU
restatement tests/support/scattered_line_reference.c on the same random
streams (checked on its own in test_scattered_line_host.py).

Tolerances are those of test_gpu_dust.py (its module docstring derives them):
the tables involve additions only and are equal to the bit; positions are
lower wall + u x cell side, no transcendental, and directions one sin / cos
each."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import line_image_lib as L
import scattered_line_lib as S
from test_gpu_dust import (SEED, _bad_pixels, _culprits, _is_threshold_case,
                           _on_box_face)

pytestmark = pytest.mark.gpu

FIELDS = S.fields()
ALBEDO = 0.6


# ------------------------------------------------------------- tables --

@pytest.mark.parametrize("name", list(FIELDS))
def test_field_tables_are_the_restatements(name):
    ncell, w = FIELDS[name]
    model = S.unit_model(ncell)
    ref = S.Restatement(model, w)
    eng = S.make_engine(model, w)
    total, B, Cs = eng.get_cell_source()
    want_total, want_B, want_C = ref.tables()
    eng.close()
    assert np.array_equal(B, want_B)
    assert np.array_equal(Cs, want_C)
    assert total == want_total
    assert want_total > 0.


def test_line_tables_come_from_the_device_emissivities():
    from test_gpu_emissivity import random_state
    from test_gpu_physics import lexington_engine
    ncell = 12
    density, temperature, x = random_state(ncell, 7)
    eng = lexington_engine(ncell)
    eng.upload_cells(density, temperature, x)
    box = L.Box((-5. * 3.086e16,) * 3, (10. * 3.086e16,) * 3, (ncell,) * 3)
    for line in ("HAlpha", "OIII_5007"):
        eng.set_cell_source_line(line)
        total, B, Cs = eng.get_cell_source()
        w = eng.compute_emissivities([line])[line]
        assert (w == 0.).sum() > 10 and (w > 0.).sum() > 1000
        model = S.Model(box.anchor, box.sides, box.ncell, density, 0., 0.5,
                        0.4, 0.3, 0.7, 0.3, 8, 8, (-1., -1.), (2., 2.))
        want_total, want_B, want_C = S.Restatement(model, w).tables()
        assert np.array_equal(B, want_B), line
        assert np.array_equal(Cs, want_C), line
        assert total == want_total, line
    eng.close()


# ------------------------------------------------------------- probes --

@pytest.fixture(scope="module")
def scene():
    """the 10 x 12 x 9 grid of the statistical identity with albedo 0.6 and
    a 24 x 24 image: engine and restatement"""
    box, model, field = S.identity_model(ALBEDO, 24, 24)
    eng = S.make_engine(model, field)
    ref = S.Restatement(model, field)
    yield model, eng, ref
    eng.close()


def test_cell_source_probe(scene):
    from cmacionize_amd import engine as E
    model, eng, ref = scene
    ref.setup()
    n = 20000
    gpu = eng.dust_probe(E.DUST_PROBE_CELL_SOURCE, SEED, 0, n)
    cpu = ref.emit(SEED, 0, n)
    assert np.array_equal(gpu[:, 0], cpu[:, 0])
    assert len(np.unique(cpu[:, 0])) > 1000
    side = model.sides.max()
    assert np.allclose(gpu[:, 1:4], cpu[:, 1:4], rtol=0., atol=1e-13 * side)
    assert np.allclose(gpu[:, 4:7], cpu[:, 4:7], rtol=0., atol=1e-15)
    # EMIT follows the selected source
    emit = eng.dust_probe(E.DUST_PROBE_EMIT, SEED, 0, n)
    assert np.array_equal(emit, gpu[:, 1:7])
    assert np.all(gpu[:, 1:4] >= model.anchor)
    assert np.all(gpu[:, 1:4] < model.anchor + model.sides)


def test_cell_source_probe_on_sparse_fields():
    """dark blocks and a single emitting cell: the same cells as the
    restatement, none of them dark"""
    from cmacionize_amd import engine as E
    for name in ("blocks 1 and 2 dark", "one cell", "4x4x4"):
        ncell, w = FIELDS[name]
        model = S.unit_model(ncell)
        ref = S.Restatement(model, w)
        eng = S.make_engine(model, w)
        gpu = eng.dust_probe(E.DUST_PROBE_CELL_SOURCE, 3, 0, 5000)
        eng.close()
        cpu = ref.emit(3, 0, 5000)
        assert np.array_equal(gpu[:, 0], cpu[:, 0]), name
        assert np.all(w[gpu[:, 0].astype(int)] > 0.), name


def test_traces(scene):
    """test_gpu_dust.py::test_traces for the cell source's instantiation"""
    from cmacionize_amd import engine as E
    model, eng, ref = scene
    ref.setup()
    d = model.describe()
    n, cap = 2000, 64
    gpu = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, 0, n, None, cap)
    cpu = ref.trace(SEED, 0, n, cap)
    assert np.all(gpu[:, 3] == 0.)
    assert cpu[:, 1].max() >= 2  # some packets scatter more than once
    assert cpu[:, 0].max() < cap
    side = model.sides.max()
    ev = np.minimum(np.minimum(cpu[:, 0], gpu[:, 0]), cap).astype(int)
    g = gpu[:, 4:].reshape(n, cap, 8)
    c = cpu[:, 4:].reshape(n, cap, 8)
    for k in np.flatnonzero(gpu[:, 0] != cpu[:, 0]):
        longer = g[k] if gpu[k, 0] > cpu[k, 0] else c[k]
        assert ev[k] < cap
        assert _on_box_face(d, longer[ev[k], 0:3]), (k, gpu[k, :4],
                                                     cpu[k, :4])
    for k in range(n):
        a, b = g[k, :ev[k]], c[k, :ev[k]]
        assert np.allclose(a[:, 0:3], b[:, 0:3], rtol=0., atol=1e-12 * side), k
        assert np.allclose(a[:, 3:7], b[:, 3:7], rtol=0.,
                           atol=1e-11 * np.abs(b[:, 3:4])), k
        assert np.allclose(a[:, 7], b[:, 7], rtol=1e-11, atol=0.), k


def test_a_packet_alone_is_the_packet_among_others(scene):
    """the guard of DESIGN.md 4.6 for the new instantiation: a lane's result
    does not depend on what the other lanes of its wave do"""
    from cmacionize_amd import engine as E
    model, eng, ref = scene
    cap = 64
    among = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, 0, 64, None, cap)
    assert among[:, 1].max() >= 2
    for k in (0, 1, 17, 31, 32, 63, int(np.argmax(among[:, 1]))):
        alone = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, k, 1, None, cap)[0]
        assert np.array_equal(alone, among[k]), k


# ------------------------------------------------- whole runs, refusals --

def test_whole_run(scene):
    """test_gpu_dust.py::test_whole_run_32's scheme: rtol 1e-9 per pixel;
    packets behind a differing pixel are bisected and shown to be threshold
    cases; equal counters when no pixel differs"""
    from cmacionize_amd import engine as E
    model, eng, ref = scene
    ref.setup()
    d = model.describe()
    N = 50000
    eng.reset_image()
    eng.dust_shoot(SEED, 0, N)
    gpu = eng.download_image()
    c = eng.get_dust_counters()
    cpu, cc = ref.shoot(SEED, 0, N)
    assert c["npackets"] == N and c["ncapped"] == 0 and cc[2] == 0
    assert c["nsource_capped"] == 0 and cc[3] == 0
    assert np.count_nonzero(cpu[0]) > 300 and cc[1] > N
    assert np.abs(cpu[1]).max() > 0. and np.abs(cpu[2]).max() > 0.
    bad = _bad_pixels(gpu, cpu)
    print("differing pixels", int(bad.sum()))
    if not np.any(bad):
        assert c["nscatter"] == cc[1]
        assert c["nsteps"] == cc[0]
        return
    culprits = []
    _culprits(eng, ref, 0, N, bad, culprits)
    assert culprits, "differing pixels without a differing packet"
    cap = 4096
    for k in culprits:
        gt = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, k, 1, None, cap)[0]
        ct = ref.trace(SEED, k, 1, cap)[0]
        assert _is_threshold_case(d, ref, gt, ct, cap), k
    ok = np.ones(N, bool)
    ok[culprits] = False
    gpu2 = np.zeros_like(gpu)
    cpu2 = np.zeros_like(cpu)
    edges = np.flatnonzero(np.diff(np.r_[0, ok.astype(int), 0]))
    for lo, hi in zip(edges[0::2], edges[1::2]):
        eng.reset_image()
        eng.dust_shoot(SEED, int(lo), int(hi - lo))
        gpu2 += eng.download_image()
        cpu2 += ref.shoot(SEED, int(lo), int(hi - lo))[0]
    assert not np.any(_bad_pixels(gpu2, cpu2))


def test_additive(scene):
    model, eng, ref = scene
    N, a = 30000, 12345
    eng.reset_image()
    eng.dust_shoot(SEED, 0, N)
    whole = eng.download_image()
    eng.reset_image()
    eng.dust_shoot(SEED, 0, a)
    eng.dust_shoot(SEED, a, N - a)
    parts = eng.download_image()
    c = eng.get_dust_counters()
    assert c["ncapped"] == 0 and c["npackets"] == N
    atol = 1e-14 * np.abs(whole[0]).max()
    assert np.allclose(parts, whole, rtol=1e-12, atol=atol)


def test_one_cell_without_dust_is_direct_light_in_its_pixels():
    ncell, w = FIELDS["one cell"]
    model = S.unit_model(ncell, 0.)
    model.nx = model.ny = 32
    eng = S.make_engine(model, w)
    ref = S.Restatement(model, w)
    N = 20000
    eng.dust_shoot(SEED, 0, N)
    image = eng.download_image()
    c = eng.get_dust_counters()
    eng.close()
    assert c["nscatter"] == 0 and c["npackets"] == N
    assert not image[1].any() and not image[2].any()
    # the cell's eight corners bound its pixels
    cell = int(np.flatnonzero(w)[0])
    idx = np.array([cell // (12 * 9), (cell // 9) % 12, cell % 9])
    side = 1. / np.array(ncell, float)
    _, ex, ey = L.axes(model.theta, model.phi)
    corners = np.array([(idx + [(k >> a) & 1 for a in range(3)]) * side
                        for k in range(8)])
    px = (corners @ ex - model.img_anchor[0]) / model.img_sides[0] * model.nx
    py = (corners @ ey - model.img_anchor[1]) / model.img_sides[1] * model.ny
    inside = np.zeros((model.nx, model.ny), bool)
    inside[int(np.floor(px.min())):int(np.floor(px.max())) + 1,
           int(np.floor(py.min())):int(np.floor(py.max())) + 1] = True
    assert image[0].any() and not image[0][~inside].any()
    assert image[0].sum() == pytest.approx(N * 0.25 / np.pi, rel=1e-12)
    # equal addends 0.25 / pi, one after the other into a pixel: every order
    # of the atomics gives the sums of the restatement's positions
    hist = np.zeros(image[0].size)
    for x in ref.emit(SEED, 0, N)[:, 1:4]:
        hist[ref.pixel(x)] += 0.25 / np.pi
    assert np.array_equal(image[0].ravel(), hist)


def test_refusals_leave_a_usable_engine():
    from cmacionize_amd import GpuEngine
    from cmacionize_amd import engine as E
    from test_gpu_emissivity import random_state
    from test_gpu_physics import lexington_engine
    lib = E.load_library()
    ncell, w = FIELDS["10x12x9"]
    model = S.unit_model(ncell, 0.5)
    eng = S.make_engine(model)

    def works():
        eng.set_cell_source_field(w)
        eng.reset_image()
        eng.dust_shoot(SEED, 0, 1000)
        assert eng.download_image()[0].sum() > 0.

    # no source yet
    assert lib.cmi_gpu_dust_shoot(eng._h, SEED, 0, 10) == S.ESTATE
    assert lib.cmi_gpu_get_cell_source(eng._h, None, None, None) == S.ESTATE
    works()
    zeros = np.zeros(model.n)
    assert lib.cmi_gpu_set_cell_source_field(eng._h, S._p(zeros)) == S.ESTATE
    assert b"nothing emits" in lib.cmi_gpu_last_error()
    # a failed call leaves no source
    assert lib.cmi_gpu_dust_shoot(eng._h, SEED, 0, 10) == S.ESTATE
    works()
    for value in (-1., float("nan"), float("inf"), -0.5e-300):
        bad = w.copy()
        bad[1079] = value
        assert lib.cmi_gpu_set_cell_source_field(eng._h, S._p(bad)) == \
            S.EINVAL, value
        assert b"negative or not finite" in lib.cmi_gpu_last_error()
        works()
    assert lib.cmi_gpu_set_cell_source_field(eng._h, None) == S.EINVAL
    assert lib.cmi_gpu_set_cell_source_line(eng._h, 42) == S.EINVAL
    assert lib.cmi_gpu_set_cell_source_line(eng._h, -1) == S.EINVAL
    assert lib.cmi_gpu_set_dust_scattering_per_hydrogen(
        eng._h, 0.4, 0.3, 0.5, -1e-30) == S.EINVAL
    works()
    eng.close()

    # a line source is stale once the cells change; a field source is not
    leng = lexington_engine(8)
    assert lib.cmi_gpu_set_cell_source_line(leng._h, 0) == S.ESTATE
    assert b"cell data" in lib.cmi_gpu_last_error()
    density, temperature, x = random_state(8, 3)
    leng.upload_cells(density, temperature, x)
    leng.set_dust_scattering_per_hydrogen(0.4, 0.3, 0.5, 1e-27)
    leng.set_ccd_image(0.7, 0.3, 8, 8, (-3e17, -3e17), (6e17, 6e17))
    leng.set_cell_source_line("HAlpha")
    leng.dust_shoot(SEED, 0, 500)
    leng.upload_cells(density, temperature, x)
    assert lib.cmi_gpu_dust_shoot(leng._h, SEED, 0, 500) == S.ESTATE
    assert b"cells changed" in lib.cmi_gpu_last_error()
    leng.set_cell_source_line("HAlpha")
    leng.dust_shoot(SEED, 0, 500)
    leng.set_cell_source_field(np.ones(512))
    leng.upload_cells(density, temperature, x)
    leng.dust_shoot(SEED, 0, 500)
    # the galaxy again (the box contains the origin); the probe of the cell
    # source needs the cell source
    leng.set_continuous_source_spiral_galaxy(1e17, 1e16, 0.2)
    assert lib.cmi_gpu_dust_probe(leng._h, E.DUST_PROBE_CELL_SOURCE, SEED, 0,
                                  0, None, S._p(np.zeros(7)), 0) == S.ESTATE
    assert leng.download_image()[0].sum() > 0.
    leng.close()

    periodic = GpuEngine((4, 4, 4), (0., 0., 0.), (1., 1., 1.), (1, 0, 0),
                         device=0)
    with pytest.raises(E.EngineError, match="periodic"):
        periodic.set_cell_source_field(np.ones(64))
    periodic.close()
    block = GpuEngine((8, 4, 4), (0., 0., 0.), (1., 1., 1.), (0, 0, 0),
                      device=0, sub_offset=(4, 0, 0), sub_ncell=(4, 4, 4))
    with pytest.raises(E.EngineError, match="decomposed"):
        block.set_cell_source_field(np.ones(64))
    assert block.n == 64
    block.close()


# ---------------------------------------------------------- end to end --

def test_scattered_images_at_albedo_0_are_the_ray_traced_ones():
    """render_scattered_line_images at albedo 0 against render_line_images
    of the same engine (same cross section, supersample 8): per pixel
    |I_mc - I_rt| <= 5 sqrt(sum of squared contributions), the variance from
    the restatement run on the device's emissivities. The inputs are those
    of test_scattered_line_host.py's identity (grid, density, view, sigma,
    packets, seed); gas of one temperature and ionisation emits H-alpha in
    proportion to the density squared, that test's field."""
    from cmacionize_amd import GpuEngine
    from test_gpu_physics import LEX
    box, model, _ = S.identity_model()
    eng = GpuEngine(tuple(int(v) for v in model.ncell), tuple(model.anchor),
                    tuple(model.sides), (0, 0, 0), device=0)
    eng.set_abundances(LEX[1:])
    x = np.full((14, model.n), 0.3)
    x[0] = 1e-3
    eng.upload_cells(model.density, np.full(model.n, 8000.), x)
    w = eng.compute_emissivities(["HAlpha"])["HAlpha"]
    ratio = w / model.density ** 2
    assert w.min() > 0. and np.allclose(ratio, ratio[0], rtol=1e-12)
    N, seed = S.IDENTITY_PACKETS, S.IDENTITY_SEED
    args = (model.theta, model.phi, model.nx, model.ny, model.img_anchor,
            model.img_sides)
    mc = eng.render_scattered_line_images(["HAlpha"], *args, N, seed,
                                          model.sigma, 0., model.g, model.p_l)
    assert mc.shape == (1, 3, model.nx, model.ny)
    assert not mc[0, 1].any() and not mc[0, 2].any()
    rt = eng.render_line_images(["HAlpha"], *args, 8, model.sigma)["HAlpha"]
    eng.close()
    ref = S.Restatement(model, w)
    image, _, squares, hits = ref.shoot(seed, 0, N, True)
    scale = ref.tables()[0] / (N * model.pixel_area)
    lit = rt > 0.
    judged = lit & (hits >= 100)
    assert lit.sum() > 100 and judged.sum() >= 0.75 * lit.sum()
    assert not mc[0, 0][~lit].any()
    z = np.abs(mc[0, 0] - rt)[judged] / (np.sqrt(squares[judged]) * scale)
    print("worst", z.max(), "rms", np.sqrt(np.mean(z ** 2)))
    assert z.max() <= 5.
    # the device's image is the restatement's, far inside the noise
    assert np.allclose(mc[0, 0], image[0] * scale, rtol=1e-6,
                       atol=1e-9 * rt.max())


FILE_NAMES = {"Halpha": "HAlpha", "OIII_5007": "OIII_5007"}


def test_driver_writes_the_scattered_images(tmp_path):
    """`cmi-gpu --emission` with `scattering: true` on the 14^3 snapshot of
    test_gpu_line_image.py's driver test: three more files per line, I the
    ABI's image with the documented scaling, the ray-traced file as without
    the switch"""
    import hdf5_mini
    import oracle_lib as o
    from test_gpu_physics import lexington_engine
    exe = S.CMI_GPU
    bench = os.path.join(S.ROOT, "benchmarks")
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

    theta, phi, nx, ny, s, sigma = 1.05, 0.5, 48, 40, 2, 2.e-27
    anchor, sides = (-1.75e17, -1.5e17), (3.5e17, 3.25e17)
    npackets, seed, albedo, g, p_l = 20000, 9, 0.54, 0.44, 0.43
    switches = "EmissivityValues:\n" + "".join(
        "  %s: true\n" % name for name in FILE_NAMES)
    block = ("EmissionImages:\n  view theta: %r radians\n"
             "  view phi: %r radians\n  image width: %d\n  image height: %d\n"
             "  anchor x: %r m\n  anchor y: %r m\n  sides x: %r m\n"
             "  sides y: %r m\n  supersampling: %d\n"
             "  dust cross section per hydrogen: %r m^2\n"
             "  filename prefix: %%s\n  output folder: %s\n" %
             (theta, phi, nx, ny, anchor[0], anchor[1], sides[0], sides[1], s,
              sigma, str(tmp_path)))
    scattering = ("  scattering: true\n  number of packets: %d\n"
                  "  random seed: %d\n  dust albedo: %r\n"
                  "  dust asymmetry: %r\n"
                  "  dust peak linear polarisation: %r\n" %
                  (npackets, seed, albedo, g, p_l))
    (tmp_path / "plain.param").write_text(switches + block % "plain")
    (tmp_path / "mc.param").write_text(switches + block % "mc" + scattering)
    for params, file in (("plain.param", plain), ("mc.param", snapshot)):
        r = subprocess.run([exe, "--emission", "--params", params, "--file",
                            file], capture_output=True, text=True,
                           cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
    assert not [n for n in os.listdir(tmp_path) if "plain" in n and
                "scattered" in n]

    f = hdf5_mini.read(plain)
    ions = ["H", "He", "C+", "C++", "N", "N+", "N++", "O", "O+", "Ne", "Ne+",
            "S+", "S++", "S+++"]
    unit_length = 0.01 * float(np.ravel(
        f["/Units"].attrs["Unit length in cgs (U_L)"])[0])
    mid = f["/PartType0/Coordinates"].data.reshape(-1, 3) * unit_length
    idx = np.floor(ncell * mid / (10. * o.PC)).astype(np.int64)
    cell = (idx[:, 0] * ncell + idx[:, 1]) * ncell + idx[:, 2]

    def placed(values):
        out = np.empty_like(values)
        out[..., cell] = values
        return out

    eng = lexington_engine(ncell)
    eng.upload_cells(
        placed(f["/PartType0/NumberDensity"].data / unit_length ** 3),
        placed(f["/PartType0/Temperature"].data * float(np.ravel(
            f["/Units"].attrs["Unit temperature in cgs (U_T)"])[0])),
        placed(np.array([f["/PartType0/NeutralFraction" + i].data
                         for i in ions])))
    want = eng.render_scattered_line_images(
        list(FILE_NAMES.values()), theta, phi, nx, ny, anchor, sides,
        npackets, seed, sigma, albedo, g, p_l)
    eng.close()
    for k, file_name in enumerate(FILE_NAMES):
        traced = open(str(tmp_path / ("mc_%s.dat" % file_name)), "rb").read()
        assert traced == open(str(tmp_path / ("plain_%s.dat" % file_name)),
                              "rb").read()
        for j, stokes in enumerate("IQU"):
            path = tmp_path / ("mc_%s_scattered_%s.dat" % (file_name, stokes))
            assert path.stat().st_size == 8 * nx * ny
            got = np.fromfile(str(path)).reshape(nx, ny)
            top = np.abs(want[k, 0]).max()
            assert top > 0.
            # the same terms, added in another order by the atomics
            assert np.allclose(got, want[k, j], rtol=1e-12,
                               atol=1e-14 * top), (file_name, stokes)
        assert np.abs(want[k, 1]).max() > 0.
