"""GPU tests of the Lyman-alpha radiation field (include/cmi_gpu.h, "Lyman
alpha radiation field"): cmi_gpu_set_lya_field, the tallies of
lya_shoot_kernel's field instantiation, cmi_gpu_download_lya_field,
cmi_gpu_lya_spin_temperature and the Python entry points - against the CPU
restatement tests/support/lya_field_reference.c on the same random streams
(checked on its own in test_lya_field_host.py) and against the identities of
the contract.

Scenes: lyman_alpha_lib.parity_scene, the 12^3 box of test_gpu_lyman_alpha.py,
and the odd grid 6 x 5 x 7 with a source in every cell, so that packets start
in boundary cells too.

Tolerances. A single packet's rows are held to lya_field_lib.row_bounds (its
docstring derives it from the arithmetic of one crossing and the bounds of the
traces, 1e-9 of a cell side and of x, times the crossings of the cell). A whole
run's rows are held to 1e-8 of the element, the components of G - which cancel
- to 1e-8 of S_H + S_d of the cell. Where two device runs must agree to the
order of the atomics, 1e-12 in the same sense. The counters are equal."""
import numpy as np
import pytest

import lya_field_lib as F
import lyman_alpha_lib as Y
from test_lya_field_host import BATCH, BATCHES, SEED as IDENTITY_SEED, SIGMAS
from test_lya_field_host import identity_batches, transparent_scene

pytestmark = pytest.mark.gpu

SEED = 7
N = 5000
VIEWS = [(1.1, 0.6), (0.3, 2.0), (np.pi / 2., 0.)]
COUNTERS = ("nsteps", "nhydrogen", "ndust", "nrejections", "natomics",
            "ncapped", "npackets")


def rows_of(eng):
    f = eng.download_lya_field()
    return np.stack([f[name] for name in F.COLUMNS], axis=1)


def run(eng, seed, first, n):
    """rows, image, cube and counters of packets [first, first + n)"""
    eng.reset_lya()
    eng.lya_shoot(seed, first, n)
    image, cube = eng.download_lya()
    return rows_of(eng), image, cube, eng.get_lya_counters()


def excess(got, ref, bound):
    """the worst |got - ref| in units of its bound (0 / 0 counts as 0)"""
    d = np.abs(got - ref)
    return float(np.where(d > 0., d / np.maximum(bound, 1e-300), 0.).max())


def order_of_the_atomics(rows):
    return F.whole_run_bounds(rows, 1e-12)


@pytest.fixture(scope="module")
def parity():
    scene, _ = Y.parity_scene()
    eng = scene.engine()
    eng.set_lya_field()
    yield scene, eng
    eng.close()


# ----------------------------------------------------- single packets --

def small_scene(view=VIEWS[0]):
    scene, _ = Y.parity_scene(ncell=(6, 5, 7), nx=7, ny=5, sigma_turb=2.0e3,
                              view=view)
    scene.field = Y._f64(np.maximum(scene.field, 0.2 * scene.field.max()))
    return scene


def test_single_packets():
    """32 packets one at a time, the field on, dust, three views: every row
    element within row_bounds, the counters the restatement's (the walk is
    shared among the views, the peel-off marches and their deposits are per
    view)"""
    scene = small_scene()
    m = scene.m
    # the packets: the first emitted in a boundary cell, the first whose first
    # event lies in its emission cell, and the next thirty
    trace, margins = Y.Restatement(scene).trace(SEED, 0, 400, 2)
    pos = trace[:, Y.HEADER:].reshape(len(trace), 2, Y.ROW)[:, :, 0:3]
    idx = np.floor((pos - m.anchor) / (m.sides / m.ncell)).astype(int)
    edge = ((idx[:, 0] == 0) | (idx[:, 0] == m.ncell - 1)).any(axis=1)
    same = (trace[:, 0] >= 2) & (idx[:, 0] == idx[:, 1]).all(axis=1)
    assert edge.any() and same.any()
    ids = [int(np.argmax(edge)), int(np.argmax(same))]
    ids += [k for k in range(400) if k not in ids][:30]
    refs = []
    per_view = []
    for view in VIEWS:
        one = small_scene(view)
        one.m.img_anchor, one.m.img_sides = m.img_anchor, m.img_sides
        ref = F.FieldRestatement(one)
        runs = [ref.shoot(SEED, k, 1, crossings=True) for k in ids]
        per_view.append(runs)
        if not refs:
            refs = runs
    eng = scene.engine(VIEWS)
    eng.set_lya_field()
    worst = 0.
    for i, k in enumerate(ids):
        assert min(r[i].margin for r in per_view) > 1e-9, k
        rows, _, _, c = run(eng, SEED, k, 1)
        ref = refs[i]
        for name in ("nhydrogen", "ndust", "nrejections", "ncapped",
                     "npackets"):
            assert c[name] == ref.counters[name], (k, name)
        assert c["natomics"] == sum(r[i].counters["natomics"]
                                    for r in per_view), k
        assert c["nsteps"] == sum(r[i].counters["nsteps"] for r in per_view) \
            - 2 * ref.march_steps, k
        bound = F.row_bounds(scene, ref.rows, ref.crossings)
        assert np.array_equal(rows == 0., ref.rows == 0.), k
        worst = max(worst, excess(rows, ref.rows, bound))
    eng.close()
    print("worst |device - restatement| / bound over 32 packets", worst,
          "events of the packets", [r.counters["nhydrogen"] +
                                    r.counters["ndust"] for r in refs])
    assert worst <= 1.
    assert sum(r.counters["ndust"] for r in refs) > 0


# ----------------------------------------------------------- whole run --

def test_whole_run(parity):
    """5e3 packets of the 12^3 scene: every row element, all seven counters,
    and image and cube within test_gpu_lyman_alpha.py's bound"""
    scene, eng = parity
    ref = F.FieldRestatement(scene).shoot(SEED, 0, N)
    rows, image, cube, c = run(eng, SEED, 0, N)
    assert ref.counters["ncapped"] == 0 and ref.counters["npackets"] == N
    assert ref.counters["nhydrogen"] > 50 * N and ref.counters["ndust"] > 0
    for name in COUNTERS:
        assert c[name] == ref.counters[name], name
    assert np.all(ref.rows[:, F.L_] > 0.)
    worst = excess(rows, ref.rows, F.whole_run_bounds(ref.rows))
    bad = np.abs(cube[0] - ref.cube) > 1e-8 * ref.image[None]
    bad_image = np.abs(image[0] - ref.image) > 1e-8 * ref.image
    print("worst row element / (1e-8 of it)", worst, "cube elements off",
          int(bad.sum()), "image", int(bad_image.sum()), "margin", ref.margin)
    assert worst <= 1.
    assert not bad.any() and not bad_image.any()


# --------------------------------------------------------- invariances --

def test_additive(parity):
    """[0, N / 2) + [N / 2, N) against [0, N): the order of the atomics"""
    scene, eng = parity
    n = 2000
    whole = run(eng, SEED, 0, n)
    eng.reset_lya()
    eng.lya_shoot(SEED, 0, n // 2)
    eng.lya_shoot(SEED, n // 2, n - n // 2)
    rows = rows_of(eng)
    assert eng.get_lya_counters() == whole[3]
    assert excess(rows, whole[0], order_of_the_atomics(whole[0])) <= 1.
    assert whole[0][:, F.N_H].sum() > 50 * n


def test_three_views_and_field_off(parity):
    """the rows do not depend on the views; image, cube and counters do not
    depend on the field"""
    scene, eng = parity
    n = 1000
    rows, image, cube, c = run(eng, SEED, 0, n)
    three = scene.engine(VIEWS)
    three.set_lya_field()
    rows3, _, _, c3 = run(three, SEED, 0, n)
    three.close()
    assert excess(rows3, rows, order_of_the_atomics(rows)) <= 1.
    assert c3["nhydrogen"] == c["nhydrogen"] and c3["ndust"] == c["ndust"]
    eng.set_lya_field(False)
    try:
        eng.reset_lya()
        eng.lya_shoot(SEED, 0, n)
        off_image, off_cube = eng.download_lya()
        assert eng.get_lya_counters() == c
    finally:
        eng.set_lya_field(True)
    assert image.sum() > 0.
    assert np.allclose(off_image, image, rtol=1e-12, atol=0.)
    assert np.allclose(off_cube, cube, rtol=1e-12, atol=1e-14 * image.max())


@pytest.mark.parametrize("views", [None, VIEWS], ids=["one", "three"])
def test_past_the_first_launch(views):
    """The field's instantiations through the chunk loop of cmi_gpu_lya_shoot
    past its first launch of 2^14 packets (N above stays below it): [0, n) in
    one call against [0, 2^14) and [2^14, n) in two, on an 8^3 grid with
    16 x 16 images. The counters are equal; rows, images and cubes differ by
    the order of the atomics."""
    first = 1 << 14
    n = first + 100
    scene, _ = Y.parity_scene(ncell=(8, 8, 8), nx=16, ny=16, tau0=30.)
    eng = scene.engine(views)
    eng.set_lya_field()
    rows, image, cube, c = run(eng, SEED, 0, n)
    eng.reset_lya()
    eng.lya_shoot(SEED, 0, first)
    eng.lya_shoot(SEED, first, n - first)
    rows2 = rows_of(eng)
    image2, cube2 = eng.download_lya()
    c2 = eng.get_lya_counters()
    eng.close()
    assert c["npackets"] == n and c["ncapped"] == 0 and c["nhydrogen"] > n
    assert c2 == c
    assert rows[:, F.L_].sum() > 0.
    assert excess(rows2, rows, order_of_the_atomics(rows)) <= 1.
    for v in range(len(image)):
        assert image[v].sum() > 0.
        atol = 1e-14 * image[v].max()
        assert np.allclose(image2[v], image[v], rtol=1e-12, atol=atol), v
        assert np.allclose(cube2[v], cube[v], rtol=1e-12, atol=atol), v


# ------------------------------------------------------------ identities --

@pytest.mark.parametrize("x_crit", [0., 3.])
@pytest.mark.parametrize("dust", [True, False])
def test_estimator_identity(dust, x_crit):
    """sum S_H against sum N_H (and S_d against N_d) on the device's own
    rows: test_lya_field_host.py's batches, seed and tolerance"""
    scene, _ = Y.parity_scene(dust=dust, x_crit=x_crit)
    eng = scene.engine()
    eng.set_lya_field()
    rows, _ = identity_batches(
        lambda first, n: (run(eng, IDENTITY_SEED, first, n)[0], None))
    eng.close()
    z_H = F.identity_sigmas(rows[:, F.S_H], rows[:, F.N_H])
    print("S_H - N_H:", z_H, "sigma")
    assert rows[:, F.N_H].min() > 0. and z_H <= SIGMAS
    if dust:
        z_d = F.identity_sigmas(rows[:, F.S_D], rows[:, F.N_D])
        print("S_d - N_d:", z_d, "sigma")
        assert rows[:, F.N_D].sum() > 100. and z_d <= SIGMAS
    else:
        assert np.all(rows[:, F.S_D] == 0.) and np.all(rows[:, F.N_D] == 0.)
    assert len(rows) == BATCHES and BATCH == 250


@pytest.mark.parametrize("ncell", [(6, 5, 7), (1, 1, 1)])
def test_a_transparent_box_tallies_the_chords(ncell):
    scene = transparent_scene(ncell)
    ref = F.FieldRestatement(scene).shoot(SEED, 0, 2000)
    eng = scene.engine()
    eng.set_lya_field()
    rows, _, _, c = run(eng, SEED, 0, 2000)
    eng.close()
    assert np.all(np.isfinite(rows)) and np.all(rows[:, 1:] == 0.)
    assert c["nhydrogen"] == 0 and c["ndust"] == 0
    assert c["nsteps"] == ref.counters["nsteps"]
    assert abs(rows[:, F.L_].sum() / ref.chord - 1.) <= 1e-12
    assert np.allclose(rows[:, F.L_], ref.rows[:, F.L_], rtol=1e-12, atol=0.)


# -------------------------------------------------------- state machine --

def test_state_machine():
    from cmacionize_amd import engine as E
    scene, _ = Y.parity_scene(ncell=(6, 5, 7), nx=7, ny=5)
    m = scene.m
    eng = scene.engine()
    lib, h = eng._lib, eng._h
    rows = np.full((m.n, 8), -7.)
    spin = np.full(m.n, -7.)

    def refused(code, rc):
        assert rc == code, (rc, lib.cmi_gpu_last_error())
        assert np.all(rows == -7.) and np.all(spin == -7.)

    def download():
        return lib.cmi_gpu_download_lya_field(h, Y._p(rows))

    def temperature(scale=1., background=2.725):
        return lib.cmi_gpu_lya_spin_temperature(h, scale, background, 1, None,
                                                Y._p(spin))

    # the field is off until it is switched on
    refused(Y.ESTATE, download())
    refused(Y.ESTATE, temperature())
    eng.set_lya_field()
    assert download() == 0 and np.all(rows == 0.)
    eng.lya_shoot(SEED, 0, 200)
    assert download() == 0 and rows[:, F.N_H].sum() > 200.
    assert temperature() == 0 and np.all(spin > 0.)
    spin[:] = -7.
    rows[:] = -7.
    for bad in ((0., 2.725), (-1., 2.725), (np.inf, 2.725), (np.nan, 2.725),
                (1., 0.), (1., -3.), (1., np.inf), (1., np.nan)):
        refused(Y.EINVAL, temperature(*bad))
    # reset_lya zeroes the rows
    eng.reset_lya()
    assert download() == 0 and np.all(rows == 0.)
    rows[:] = -7.
    # off again: freed
    eng.set_lya_field(False)
    refused(Y.ESTATE, download())
    # the mode set anew switches the field off
    eng.set_lya_field()
    scene.apply(eng)
    refused(Y.ESTATE, download())
    # a stale mode
    eng.set_lya_field()
    eng.set_cell_source_field(scene.field)
    refused(Y.ESTATE, download())
    refused(Y.ESTATE, temperature())
    # a capped packet
    eng.set_lyman_alpha(scene.nchan, scene.vmin, scene.vmax, 0., 0., 2,
                        scene.n_HI, scene.T)
    eng.set_lya_field()
    eng.lya_shoot(SEED, 0, 100)
    assert eng.get_lya_counters()["ncapped"] > 0
    refused(Y.ESTATE, download())
    refused(Y.ESTATE, temperature())
    assert b"cap" in lib.cmi_gpu_last_error()
    # core skipping: the rows are there, the spin temperature is refused
    eng.set_lyman_alpha(scene.nchan, scene.vmin, scene.vmax, 0., 3.,
                        Y.MAX_SCATTER, scene.n_HI, scene.T)
    eng.set_lya_field()
    eng.lya_shoot(SEED, 0, 100)
    assert download() == 0 and rows[:, F.N_H].sum() > 0.
    rows[:] = -7.
    refused(Y.ESTATE, temperature())
    assert b"core skipping" in lib.cmi_gpu_last_error()
    with pytest.raises(E.EngineError, match="core skipping"):
        eng.lya_spin_temperature(100, 2.725)
    assert eng.lya_radiation_field(100)["scattering_rate"] is None
    # the mode off
    eng.set_lyman_alpha(0, 0., 1.)
    refused(Y.ESTATE, lib.cmi_gpu_set_lya_field(h, 1))
    # a point camera: the mode is refused, and so is the field
    eng.set_sky_camera(m.anchor + 0.5 * m.sides, 8, 4,
                       float(m.sides.min()) / 50.)
    with pytest.raises(E.EngineError):
        scene.apply(eng)
    refused(Y.ESTATE, lib.cmi_gpu_set_lya_field(h, 1))
    eng.close()
    # a block of a decomposed grid
    block = E.GpuEngine((8, 4, 4), (0., 0., 0.), (1., 1., 1.), (0, 0, 0),
                        device=0, sub_offset=(4, 0, 0), sub_ncell=(4, 4, 4))
    block.upload_cells(np.full(64, 1e8), np.full(64, 100.),
                       np.ones((E.NION, 64)))
    assert lib.cmi_gpu_set_lyman_alpha(block._h, 16, -1e5, 1e5, 0., 0., 1000,
                                       None, None) == Y.ESTATE
    assert lib.cmi_gpu_set_lya_field(block._h, 1) == Y.ESTATE
    block.close()


# ------------------------------------------------- coupling end to end --

T_GAMMA = 2.725
A_HE = 0.1


def test_coupling_end_to_end():
    """T_s of lya_spin_temperature against the restatement's on the same
    packets, and what render_hi_cube makes of it"""
    from cmacionize_amd import engine as E
    scene, _ = Y.parity_scene()
    m = scene.m
    n_HI, T = scene.n_HI.reshape(-1), scene.T.reshape(-1).copy()
    T[5] = 0.  # a cell without a temperature
    x = np.zeros((E.NION, m.n))
    x[0] = n_HI / m.density
    x[1] = 0.3
    eng = scene.engine()
    eng.upload_cells(m.density, T, x)
    eng.set_abundances([A_HE, 2.2e-4, 4.0e-5, 3.3e-4, 5.0e-5, 9.0e-6])
    eng.set_cell_source_field(scene.field)
    scene.apply(eng)
    eng.set_lya_field()
    n = 2000
    eng.lya_shoot(SEED, 0, n)
    ref_scene, _ = Y.parity_scene()
    ref = F.FieldRestatement(ref_scene)
    run_ = ref.shoot(SEED, 0, n)
    # a luminosity that puts x_alpha near 1 in the middle of the box
    total = eng.get_cell_source(tables=False)
    P1 = ref.scattering_rate(run_.rows, total / n)
    scale = 27. * E.HI_EINSTEIN_A * T_GAMMA / (4. * F.T_STAR) / np.median(P1)
    luminosity = total * scale
    P_ref = ref.scattering_rate(run_.rows, luminosity / n)
    n_e = m.density * ((1. - x[0]) + A_HE * (1. - x[1]))
    for collisions in (True, False):
        P, T_s = eng.lya_spin_temperature(n, T_GAMMA, collisions, luminosity)
        T_ref = F.spin_temperature_c(T, n_HI, n_e, P_ref, T_GAMMA, collisions)
        worst = (np.abs(P / P_ref - 1.).max(), np.abs(T_s / T_ref - 1.).max())
        print("collisions", collisions, "worst relative P, T_s", worst)
        # P is S_H of the cell times constants; |d ln T_s / d ln x| <= 1
        assert worst[0] <= 1e-8 and worst[1] <= 2e-8
        assert T_s[5] == T_GAMMA
    field = eng.lya_radiation_field(n, luminosity)
    assert np.array_equal(field["scattering_rate"], P)
    V = F.cell_volume(m)
    assert np.allclose(field["energy_density"], run_.rows[:, F.L_] *
                       luminosity / n / (E.LIGHTSPEED * V), rtol=1e-8,
                       atol=0.)
    assert field["force"].shape == (3, m.n)
    # the coupled cube lies between the kinetic one and none at all, and
    # differs from the kinetic one where the coupling is weak
    # (without the collisions: at this density they alone couple every cell)
    P, T_s = eng.lya_spin_temperature(n, T_GAMMA, False, luminosity)
    xc = F.coupling(np.maximum(T, 1.), n_HI, n_e, T_GAMMA, False, P)
    assert (xc < 1.).any() and (xc > 1.).any()
    args = (m.theta, m.phi, m.nx, m.ny, m.img_anchor, m.img_sides, 8, -4.0e4,
            4.0e4)
    hi = dict(sigma_turb=2.0e3, background_temperature=T_GAMMA)
    T_k = np.where(T > 0., T, T_GAMMA)
    kinetic = eng.render_hi_cube(*args, spin_temperature=T_k, **hi)
    coupled = eng.render_hi_cube(*args, spin_temperature=T_s, **hi)
    weak = np.where(xc < 1., T_k, T_s)
    partly = eng.render_hi_cube(*args, spin_temperature=weak, **hi)
    assert not np.array_equal(coupled, kinetic)
    # with T_k put back into the weakly coupled cells, less of the
    # difference is left than with the coupling everywhere
    assert np.abs(partly - kinetic).sum() < np.abs(coupled - kinetic).sum()
    # render_lyman_alpha_cube hands the field out, and returns what it did
    images = eng.render_lyman_alpha_cube(
        m.theta, m.phi, m.nx, m.ny, m.img_anchor, m.img_sides, 500, SEED,
        scene.nchan, scene.vmin, scene.vmax, sigma_turb=2.0e3,
        source=scene.field)
    with_field = eng.render_lyman_alpha_cube(
        m.theta, m.phi, m.nx, m.ny, m.img_anchor, m.img_sides, 500, SEED,
        scene.nchan, scene.vmin, scene.vmax, sigma_turb=2.0e3,
        source=scene.field, field=True)
    assert len(images) == 2 and len(with_field) == 3
    assert np.allclose(with_field[0], images[0], rtol=1e-12, atol=0.)
    assert set(with_field[2]) == {"energy_density", "scattering_rate",
                                  "force"}
    assert with_field[2]["energy_density"].min() >= 0.
    assert with_field[2]["energy_density"].max() > 0.
    eng.close()
