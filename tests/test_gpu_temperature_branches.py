"""Every branch of the temperature solve through every device form of it:
the lattice of tests/temperature_lattice.py (synthetic cells that the oracle
shows to take each branch of TemperatureCalculator::calculate_temperature,
with and without cosmic ray heating, on a grid whose z layers differ) uploaded
as cells plus accumulators and updated by

  temperature_kernel                     temperature_pipeline=0
  the pipeline's default mix
  eval / linecool / secant steps only    temperature_finish_slots=0
  temp_finish_kernel only                temperature_finish_slots > cells
  thermal_probe_kernel                   thermal_probe(1, ...)

which must agree bit for bit, and with the oracle at the project's tolerances
(T 1e-6, fractions 1e-5) in every cell the oracle itself finds
well-conditioned."""
import time

import numpy as np
import pytest

import temperature_lattice as tl

pytestmark = pytest.mark.gpu

# (name, tuning) in the order they run on one engine: the default first
TUNINGS = [
    ("default", dict()),
    ("steps_only", dict(temperature_pipeline=1, temperature_finish_slots=0)),
    ("finish_only", dict(temperature_pipeline=1,
                         temperature_finish_slots=1 << 20)),
    ("one_kernel", dict(temperature_pipeline=0)),
]
assert 1 << 20 > tl.N


def lattice_engine(crfac, sub_offset=None, sub_ncell=None):
    from cmacionize_amd import GpuEngine
    eng = GpuEngine(tl.NCELL, tl.ANCHOR, tl.SIDES, (0, 0, 0), device=0,
                    track_heating=True, sub_offset=sub_offset,
                    sub_ncell=sub_ncell)
    eng.set_sources([[0.5 * tl.SIDES[0], 0.5 * tl.SIDES[1], 0.]], [1.],
                    tl.LUMINOSITY)
    eng.set_spectrum_planck(40000.)
    eng.set_cross_sections_verner()
    eng.set_recombination_rates_verner()
    eng.set_abundances(tl.ABUNDANCES)
    eng.set_temperature_params(
        do_temperature_calculation=1,
        minimum_number_of_iterations=tl.MIN_ITERATION,
        epsilon_convergence=tl.EPSILON,
        maximum_number_of_iterations=tl.MAX_ITERATIONS,
        pah_heating_factor=tl.PAHFAC,
        cosmic_ray_heating_factor=crfac,
        cosmic_ray_heating_limit=tl.CRLIM,
        cosmic_ray_heating_scale_length=tl.CRSCALE,
        minimum_ionized_temperature=tl.T_MIN_IONIZED)
    eng.reset_grid()
    return eng


def upload(eng, select=None):
    """The lattice's state and accumulators (of the cells `select`)."""
    from cmacionize_amd import engine as E
    cell = tl.cells()
    pick = (lambda a: a) if select is None else (lambda a: a[..., select])
    eng.upload_cells(pick(cell.number_density), pick(cell.temperature),
                     np.ascontiguousarray(pick(cell.x)))
    for ion in range(14):
        eng.upload_field(E.FIELD_MEAN_INTENSITY + ion, pick(cell.J[ion]))
    for k in range(2):
        eng.upload_field(E.FIELD_HEATING + k, pick(cell.heating[k]))


def download(eng):
    """(T[n], x[14][n], heating[2][n]) as one [17][n] array"""
    from cmacionize_amd import engine as E
    out = [eng.download_field(E.FIELD_TEMPERATURE)]
    out += [eng.download_field(E.FIELD_IONIC_FRACTION + ion)
            for ion in range(14)]
    out += [eng.download_field(E.FIELD_HEATING + k) for k in range(2)]
    return np.array(out)


def same_bits(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def runs():
    """{crfac: {tuning name: [17][N] result}}: both models under the four
    tunings, state and accumulators uploaded afresh before each update."""
    out = {}
    for crfac in (0., 1.):
        eng = lattice_engine(crfac)
        out[crfac] = {}
        for name, tuning in TUNINGS:
            eng.set_tuning(**tuning)
            upload(eng)
            start = time.perf_counter()
            eng.update_cells(tl.LOOP_TEMPERATURE, tl.TOTWEIGHT)
            eng.synchronize()
            print("crfac %g %-12s update of %d cells: %.3f s" % (
                crfac, name, tl.N, time.perf_counter() - start))
            out[crfac][name] = download(eng)
            out[crfac][name].setflags(write=False)
        eng.close()
    return out


@pytest.mark.parametrize("crfac", [0., 1.])
def test_four_paths_give_the_same_bits(runs, crfac):
    """temperature, 14 fractions and both heating terms of every cell -
    ill-conditioned ones included"""
    ref = runs[crfac]["one_kernel"]
    assert np.isfinite(ref).all()
    for name, _ in TUNINGS:
        got = runs[crfac][name]
        differ = np.flatnonzero((got != ref).any(axis=0))
        assert same_bits(got, ref), (
            name, len(differ), differ[:8], got[:3, differ[:4]],
            ref[:3, differ[:4]])


@pytest.mark.parametrize("crfac", [0., 1.])
def test_device_solve_matches_oracle(oracle, runs, crfac):
    s = tl.solved(crfac)
    got = runs[crfac]["default"]
    T, x, heating = got[0], got[1:15], got[15:17]
    well = ~s.ill
    errT = np.abs(T - s.T) / s.T
    nz = s.x != 0.
    errx = np.zeros_like(x)
    errx[nz] = np.abs(x[nz] - s.x[nz]) / np.abs(s.x[nz])
    errx[~nz] = np.where(x[~nz] == 0., 0., np.inf)
    print("crfac %g: worst device / oracle - 1 of the %d well-conditioned "
          "cells: T %.3g (of 1e-6), fractions %.3g (of 1e-5); of the %d "
          "ill-conditioned: T %.3g, fractions %.3g" % (
              crfac, np.count_nonzero(well), errT[well].max(),
              errx[:, well].max(), np.count_nonzero(s.ill),
              errT[s.ill].max() if s.ill.any() else 0.,
              errx[:, s.ill].max() if s.ill.any() else 0.))
    # exact where the contract is exact: cells that take no solve ...
    neutral = s.nsteps == 0
    assert neutral.sum() >= 28
    assert (T[neutral] == 500.).all()
    assert (x[:2, neutral] == 1.).all() and (x[2:, neutral] == 0.).all()
    assert (heating[:, neutral] == 0.).all()
    # ... the normalised heating terms (one product, hfac x heating) ...
    assert np.array_equal(heating, s.heating)
    # ... and the clamps of the solve: the 30000 K cap, h0 = 1 (T below
    # t_min_ionized, or J_H = 0) and h0 <= 1e-10 (T above 1e10 K) with their
    # zeroed metals. (Whether an ill-conditioned cell ends in a clamp is as
    # uncertain as its temperature.)
    capped = (s.T == 30000.) & well
    assert capped.sum() >= 8 and (T[capped] == 30000.).all()
    assert np.array_equal((x[0] == 1.)[well], (s.x[0] == 1.)[well])
    assert np.array_equal((x[0] <= 1.e-10)[well], (s.x[0] <= 1.e-10)[well])
    clamped = ((s.x[0] == 1.) | (s.x[0] <= 1.e-10)) & well
    assert clamped.sum() >= 8 and (x[2:, clamped] == 0.).all()
    hot = (s.x[0] == 1.e-10) & well  # (T > 1e10 K sets both to 1e-10)
    assert hot.sum() >= 8 and np.array_equal(x[:2, hot], s.x[:2, hot])
    # the project's tolerances (test_lexington_iteration_matches_oracle)
    bad = well & ~np.isclose(T, s.T, rtol=1e-6, atol=0.)
    assert not bad.any(), (np.flatnonzero(bad)[:8], T[bad][:8], s.T[bad][:8])
    for ion in range(14):
        bad = well & ~np.isclose(x[ion], s.x[ion], rtol=1e-5, atol=1e-300)
        assert not bad.any(), (ion, np.flatnonzero(bad)[:8], x[ion][bad][:8],
                               s.x[ion][bad][:8])


@pytest.mark.parametrize("crfac", [0., 1.])
def test_helium_of_cells_without_neutral_oxygen_radiation(runs, crfac):
    """J(O0) = 0 with J_He > 0: "J_He == 0 -> he0 = 1" at the end of the solve
    has to look at helium's accumulator, wherever the layout keeps it - x(He0)
    is the oracle's, not 1."""
    cell = tl.cells()
    s = tl.solved(crfac)
    pick = (cell.variant == tl.VARIANTS.index("JO0_zero")) & ~s.ill & \
        (s.nsteps > 0)
    assert (cell.J[tl.ION_O_n][pick] == 0.).all()
    assert (cell.J[tl.ION_He_n][pick] > 0.).all()
    ionized = pick & (s.x[1] < 1.)
    assert ionized.sum() >= 100
    for name, _ in TUNINGS:
        he0 = runs[crfac][name][2]
        forced = np.flatnonzero(ionized & (he0 == 1.))
        assert len(forced) == 0, (name, len(forced), forced[:8],
                                  s.x[1][forced[:8]])
        assert np.allclose(he0[pick], s.x[1][pick], rtol=1e-5, atol=1e-300)


def test_block_of_the_grid_gives_the_whole_grids_bits(runs):
    """an engine that holds the block [5, 25) x [0, 39) x [1, 4) of the grid:
    its cells' z - the cosmic ray heating's exp(-|z| / crscale) - come from
    the block's offset"""
    offset, ncell = (5, 0, 1), (20, 39, 3)
    ix, iy, iz = np.meshgrid(*[offset[a] + np.arange(ncell[a])
                               for a in range(3)], indexing="ij")
    select = ((ix * tl.NCELL[1] + iy) * tl.NCELL[2] + iz).ravel()
    assert len(select) % 64 != 0
    eng = lattice_engine(1., sub_offset=offset, sub_ncell=ncell)
    assert eng.n == len(select)
    whole = runs[1.]["default"]
    for name, tuning in TUNINGS:
        eng.set_tuning(**tuning)
        upload(eng, select)
        eng.update_cells(tl.LOOP_TEMPERATURE, tl.TOTWEIGHT)
        eng.synchronize()
        got = download(eng)
        differ = np.flatnonzero((got != whole[:, select]).any(axis=0))
        assert same_bits(got, whole[:, select]), (name, len(differ),
                                                  differ[:8])
    eng.close()


def test_update_in_two_ranges_gives_the_single_calls_bits(runs):
    split = 2477
    assert split % 64 != 0 and 0 < split < tl.N
    eng = lattice_engine(1.)
    for name, tuning in TUNINGS:
        eng.set_tuning(**tuning)
        upload(eng)
        eng.update_cells_range(tl.LOOP_TEMPERATURE, tl.TOTWEIGHT, split,
                               tl.N - split)
        eng.update_cells_range(tl.LOOP_TEMPERATURE, tl.TOTWEIGHT, 0, split)
        eng.synchronize()
        assert same_bits(download(eng), runs[1.]["default"]), name
    eng.close()


def test_probe_gives_the_update_kernels_bits(runs):
    """thermal_probe_kernel (temperature_cell on rows of normalised integrals)
    against the cell update. The grid normalises J with exactly 1; the
    normalised heating terms are the oracle's (equal to the device's bit for
    bit, test_device_solve_matches_oracle)."""
    cell = tl.cells()
    s = tl.solved(0.)
    eng = lattice_engine(0.)
    x, T, h = eng.thermal_probe(
        1, np.ascontiguousarray(cell.J.T),
        np.ascontiguousarray(s.heating.T),
        cell.temperature, cell.number_density)
    eng.close()
    got = np.vstack([T[None, :], x.T, h.T])
    ref = runs[0.]["default"]
    differ = np.flatnonzero((got != ref).any(axis=0))
    assert same_bits(got, ref), (len(differ), differ[:8])


def test_ionization_balance_of_the_lattice(oracle):
    """the same cells at a loop that solves no temperature:
    `ionization_kernel<FULL>` with J_H = 0, J_He = 0, no radiation and vacuum
    among them, against the oracle at the tolerance of
    test_ionization_state_calculator_on_device (1e-9, as rel_ok measures it)
    in the cells the oracle pins down to a tenth of that"""
    want = tl.ionized(0.)
    eng = lattice_engine(0.)
    upload(eng)
    eng.update_cells(tl.LOOP_IONIZATION, tl.TOTWEIGHT)
    eng.synchronize()
    got = download(eng)
    eng.close()
    T, x = got[0], got[1:15]
    assert np.array_equal(T, tl.cells().temperature)
    # (the reference's 0 / 0 for the metals of a cell without electrons)
    assert np.array_equal(np.isnan(x), np.isnan(want.x))
    both = np.abs(x + want.x)
    err = np.where(np.isnan(want.x) | (x == want.x), 0.,
                   np.abs(x - want.x) / np.where(both > 0., both, 1.))
    well = ~want.ill
    print("ionization balance: worst |a - b| / |a + b| of the %d "
          "well-conditioned cells %.3g (of 1e-9), of the %d others %.3g" % (
              np.count_nonzero(well), err[:, well].max(),
              np.count_nonzero(want.ill), err[:, want.ill].max()))
    bad = well & (err > tl.IONIZATION_TOLERANCE).any(axis=0)
    assert not bad.any(), (np.flatnonzero(bad)[:8], err[:, bad].max(axis=0)[:8])
    # no solve, nothing to condition: neutral without hydrogen-ionizing
    # radiation, empty in vacuum
    dark = (tl.cells().J[0] == 0.) & (tl.cells().number_density > 0.)
    vacuum = tl.cells().number_density == 0.
    assert dark.sum() >= 1280 and vacuum.sum() >= 18
    assert np.array_equal(x[:, dark], want.x[:, dark])
    assert np.array_equal(x[:, vacuum], want.x[:, vacuum])
