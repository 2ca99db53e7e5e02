"""The hydrogen-only cell update with the temperature-only terms of the metals'
balance shared by the rows of 64 cells that have one temperature
(`update_reuse=1`, the default) against the same update with every cell
evaluating them for itself (`update_reuse=0`): the same functions on the same
values, so every ionic fraction and heating term must be equal bit for bit,
whatever the pattern of temperatures - and against the oracle's update."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# 6144 cells = 96 full rows, 12 chunks of 8 rows; 2860 cells = 44 rows and a
# row of 44 cells, the last chunk has 5 rows
SHAPES = [(24, 16, 16), (20, 13, 11)]
ROW = 64
CHUNK = 8 * ROW
TOTWEIGHT = 1.e5


def temperatures(pattern, n):
    rng = np.random.default_rng(7)
    T = np.full(n, 8000.)
    if pattern == "uniform":
        pass
    elif pattern == "slabs_row_boundary":
        # inside the fourth chunk, between its third and fourth row
        T[3 * CHUNK + 3 * ROW:] = 11000.
    elif pattern == "slabs_mid_row":
        T[3 * CHUNK + 3 * ROW + 20:] = 11000.
    elif pattern == "every_cell":
        T = rng.uniform(5000., 15000., n)
    elif pattern == "one_cell_last_chunk":
        last_chunk = ((n + ROW - 1) // ROW - 1) // 8 * CHUNK
        assert last_chunk < n - 10
        T[n - 10] = 9500.
    else:
        raise ValueError(pattern)
    return T


def state(n):
    """Seeded mean intensities (a fifth of them zero) and heating terms, and a
    density with vacuum cells - some of them in rows of their own."""
    rng = np.random.default_rng(11)
    J = 10. ** rng.uniform(-9., -1., n)
    J[rng.random(n) < 0.2] = 0.
    J[5 * ROW:7 * ROW] = 0.  # two rows where no cell needs any term
    heating = 10. ** rng.uniform(-30., -20., (2, n))
    density = np.full(n, 100. * 1.e6)
    density[rng.random(n) < 0.1] = 0.
    density[9 * ROW + 7:10 * ROW + 9] = 0.
    return J, heating, density


def make_engine(shape, track_heating, verner_rates=False):
    from cmacionize_amd import GpuEngine, STROMGREN as S
    eng = GpuEngine(shape, S["anchor"], S["sides"], S["periodic"], device=0,
                    track_heating=track_heating)
    eng.set_sources(S["source_position"], S["source_weight"], S["luminosity"])
    eng.set_spectrum_monochromatic(S["frequency"])
    sigma = np.zeros(14)
    sigma[0] = S["sigma_H"]
    eng.set_cross_sections_fixed(sigma)
    if verner_rates:
        eng.set_recombination_rates_verner()
    else:
        alpha = np.zeros(14)
        alpha[0] = S["alpha_H"]
        eng.set_recombination_rates_fixed(alpha)
    return eng


def run_update(eng, reuse, density, T, J, heating, track_heating):
    """One update from the same uploaded state; all the fields it writes."""
    from cmacionize_amd import engine as E
    n = density.size
    x = np.zeros((14, n))
    x[0] = 1.e-6
    x[1] = 1.e-6
    eng.upload_cells(density, T, x)
    eng.upload_field(E.FIELD_MEAN_INTENSITY, J)
    if track_heating:
        for k in range(2):
            eng.upload_field(E.FIELD_HEATING + k, heating[k])
    eng.set_tuning(update_reuse=reuse)
    eng.update_cells(0, TOTWEIGHT)
    eng.synchronize()
    out = [eng.download_field(E.FIELD_IONIC_FRACTION + i) for i in range(14)]
    if track_heating:
        out += [eng.download_field(E.FIELD_HEATING + k) for k in range(2)]
    return out


def same_bits(a, b):
    """np.array_equal, and NaN payloads and signs of zero as well."""
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("track_heating", [False, True])
@pytest.mark.parametrize("pattern", [
    "uniform", "slabs_row_boundary", "slabs_mid_row", "every_cell",
    "one_cell_last_chunk"])
@pytest.mark.parametrize("shape", SHAPES)
def test_reuse_equals_per_lane_update(oracle, shape, pattern, track_heating):
    n = int(np.prod(shape))
    T = temperatures(pattern, n)
    J, heating, density = state(n)
    eng = make_engine(shape, track_heating)
    with_reuse = run_update(eng, 1, density, T, J, heating, track_heating)
    without = run_update(eng, 0, density, T, J, heating, track_heating)
    eng.close()
    for k, (a, b) in enumerate(zip(with_reuse, without)):
        assert same_bits(a, b), (k, int((a != b).sum()))
    xH = with_reuse[0]
    ionized = (J > 0.) & (density > 0.)
    assert (xH[ionized] < 1.).all() and (xH[~ionized & (density > 0.)] == 1.).all()
    assert (xH[density == 0.] == 0.).all()
    if track_heating:
        assert not same_bits(with_reuse[14], heating[0])  # normalised in place
    if pattern == "uniform":
        # the oracle's update of the same state (test_gpu_physics.py: the
        # closed form of the hydrogen balance is equal bit for bit)
        from cmacionize_amd import STROMGREN as S
        sim = oracle.OracleSimulation(shape, S["anchor"], S["sides"])
        sim.set_sources(S["source_position"], S["source_weight"],
                        S["luminosity"])
        m = sim.model
        m.spectrum_type = oracle.SPECTRUM_MONOCHROMATIC
        m.mono_frequency = S["frequency"]
        m.xsec_type = oracle.XSEC_FIXED
        m.xsec_fixed[0] = S["sigma_H"]
        m.recomb_type = oracle.RECOMB_FIXED
        m.recomb_fixed[0] = S["alpha_H"]
        m.reemit_type = oracle.REEMIT_NONE
        m.do_temperature = 0
        sim.number_density[:] = density
        sim.temperature[:] = T
        sim.J[0][:] = J
        sim.heating[:] = heating
        sim.update(0, TOTWEIGHT)
        assert np.array_equal(xH, sim.x[0])


@pytest.mark.parametrize("pattern", ["uniform", "slabs_mid_row", "every_cell"])
def test_reuse_equals_per_lane_update_with_fitted_rates(oracle, pattern):
    """... and with recombination rates that do depend on the temperature
    (the Verner fits): stored for one temperature, never used for another.
    The uniform case - every row on the stored terms - also against the
    oracle's update, the metals' fractions included, at the tolerance of
    test_gpu_physics.py's balance (device exp / log differ from libm by
    ulps)."""
    shape = SHAPES[1]
    n = int(np.prod(shape))
    T = temperatures(pattern, n)
    J, heating, density = state(n)
    eng = make_engine(shape, True, verner_rates=True)
    with_reuse = run_update(eng, 1, density, T, J, heating, True)
    without = run_update(eng, 0, density, T, J, heating, True)
    eng.close()
    for k, (a, b) in enumerate(zip(with_reuse, without)):
        assert same_bits(a, b), (k, int((a != b).sum()))
    if pattern == "uniform":
        from cmacionize_amd import STROMGREN as S
        sim = oracle.OracleSimulation(shape, S["anchor"], S["sides"])
        sim.set_sources(S["source_position"], S["source_weight"],
                        S["luminosity"])
        m = sim.model
        m.spectrum_type = oracle.SPECTRUM_MONOCHROMATIC
        m.mono_frequency = S["frequency"]
        m.xsec_type = oracle.XSEC_FIXED
        m.xsec_fixed[0] = S["sigma_H"]
        m.recomb_type = oracle.RECOMB_VERNER
        m.reemit_type = oracle.REEMIT_NONE
        m.do_temperature = 0
        sim.number_density[:] = density
        sim.temperature[:] = T
        sim.J[0][:] = J
        sim.heating[:] = heating
        sim.update(0, TOTWEIGHT)
        for ion in range(14):
            want = np.asarray(sim.x[ion])
            print(ion, np.nanmax(np.abs(with_reuse[ion] - want) /
                                 np.maximum(np.abs(want), 1e-300)))
            assert np.allclose(with_reuse[ion], want, rtol=1e-8, atol=1e-14,
                               equal_nan=True), ion
