"""A lattice of synthetic cells that drives every branch of the temperature
solve (TemperatureCalculator::calculate_temperature,
src/TemperatureCalculator.cpp:567-931), solved by the oracle. Pure numpy plus
the oracle: no GPU.

Base rows: rows 0, 25, 50, 75 of tests/golden/tbal_testdata.txt (columns 0-13
the 14 mean intensities, columns 14-15 x 1e-7 the heating terms). Base row r is
the z layer r of a grid with four cells in z, so every row sees its own
exp(-|z| / crscale) of the cosmic ray heating. Per base row

  10 scales of J and heating together   10^-10, 10^-8, ..., 10^8
   4 densities                          1e2, 1e5, 1e7, 1e9 m^-3
   2 input temperatures                 100 K (restart at 8000 K), 9000 K
   4 further factors on the heating     0, 1, 1e4, -1
   4 variants                           as is, J_He = 0, J_H = 0, J(O0) = 0

= 1280 cells, 5120 in all, followed by 28 special cells (vacuum with and
without radiation, matter without radiation): 5148 cells, not a multiple of
the wave size.

The grid's cells are 1 m x 1 m x 0.75 scale lengths, the luminosity is the
cell volume in photons per second and the total weight is 1, so that the
oracle's own grid-level update (cmio_update_cells) normalises J with exactly 1
and computes hfac and the cells' z itself; the layers' midpoints are at -0.25,
0.5, 1.25 and 2 scale lengths.

Conditioning is decided by the oracle alone: a cell is ill-conditioned if
multiplying J and heating by 1 + 1e-13 u (u uniform in [-1, 1], two draws) moves
the oracle's temperature by more than 1e-7 or any fraction by more than 1e-6
relative - a tenth of the tolerances of test_lexington_iteration_matches_oracle
- or changes the number of secant steps or the branches the solve takes.
Such cells are excused from the device-versus-oracle tolerance, nothing else.
"""
import functools
import os
from types import SimpleNamespace

import numpy as np

import oracle_lib as o

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

BASE_ROWS = (0, 25, 50, 75)
SCALES = tuple(10. ** e for e in range(-10, 10, 2))
DENSITIES = (1.e2, 1.e5, 1.e7, 1.e9)
TEMPERATURES = (100., 9000.)
HEATING_FACTORS = (0., 1., 1.e4, -1.)
VARIANTS = ("as_is", "JHe_zero", "JH_zero", "JO0_zero")
ION_H_n, ION_He_n, ION_O_n = 0, 1, 7

NLATTICE = len(BASE_ROWS) * len(SCALES) * len(DENSITIES) * \
    len(TEMPERATURES) * len(HEATING_FACTORS) * len(VARIANTS)
# the grid: 33 x 39 x 4 = 5148 cells = 5120 + 28 special cells
NCELL = (33, 39, 4)
N = NCELL[0] * NCELL[1] * NCELL[2]
assert NLATTICE == 5120 and N > NLATTICE and N % 64 != 0

CRSCALE = 1.33333 * 3.086e19      # the engine's default scale length (m)
CRLIM = 0.75                      # ... and neutral-fraction limit
CELLSIDE_Z = 0.75 * CRSCALE
ANCHOR = (0., 0., -0.25 * CRSCALE - 0.5 * CELLSIDE_Z)
SIDES = (float(NCELL[0]), float(NCELL[1]), 4. * CELLSIDE_Z)
LUMINOSITY = CELLSIDE_Z           # = the cell volume: jfac = 1
TOTWEIGHT = 1.
ABUNDANCES = (0.1, 2.2e-4, 4.e-5, 3.3e-4, 5.e-5, 9.e-6)  # He C N O Ne S
PAHFAC, EPSILON, MAX_ITERATIONS, T_MIN_IONIZED = 1., 1.e-3, 100, 4000.
MIN_ITERATION = 3
LOOP_TEMPERATURE = MIN_ITERATION + 2   # a loop that solves the temperature
LOOP_IONIZATION = MIN_ITERATION        # ... and one that does not

CONDITION_PERTURBATION = 1.e-13
CONDITION_T, CONDITION_X = 1.e-7, 1.e-6
MAX_ILL_SHARE = 0.03
IONIZATION_TOLERANCE = 1.e-9  # test_ionization_state_calculator_on_device
CONDITION_X_IONIZATION = 0.1 * IONIZATION_TOLERANCE


def _load(name):
    rows = []
    for line in open(os.path.join(GOLDEN, name)):
        if line.lstrip().startswith("#") or not line.strip():
            continue
        rows.append([float(v) for v in line.split()])
    return np.array(rows)


@functools.lru_cache(maxsize=None)
def cells():
    """The lattice's inputs: J[14][N], heating[2][N] (un-normalised, as the
    accumulators hold them), number_density[N], temperature[N], x[14][N], and
    variant[N] (index into VARIANTS; -1 for the special cells)."""
    data = _load("tbal_testdata.txt")
    J = np.zeros((o.NION, N))
    heating = np.zeros((2, N))
    density = np.zeros(N)
    temperature = np.zeros(N)
    variant = np.full(N, -1)
    k = 0  # index inside a z layer: cell 4 k + r belongs to base row r
    for scale in SCALES:
        for n in DENSITIES:
            for T in TEMPERATURES:
                for hfactor in HEATING_FACTORS:
                    for v in range(len(VARIANTS)):
                        for r, row in enumerate(BASE_ROWS):
                            c = 4 * k + r
                            J[:, c] = data[row, :14] * scale
                            # (the update multiplies by ~ the Planck constant)
                            heating[:, c] = data[row, 14:16] * 1.e-7 * scale \
                                * hfactor / o.PLANCK
                            if VARIANTS[v] == "JHe_zero":
                                J[ION_He_n, c] = 0.
                            elif VARIANTS[v] == "JH_zero":
                                J[ION_H_n, c] = 0.
                            elif VARIANTS[v] == "JO0_zero":
                                J[ION_O_n, c] = 0.
                            density[c] = n
                            temperature[c] = T
                            variant[c] = v
                        k += 1
    assert 4 * k == NLATTICE
    # special cells: 10 vacuum cells without radiation, 10 cells of matter
    # without radiation, 8 vacuum cells with radiation
    c = NLATTICE
    for j in range(N - NLATTICE):
        row = BASE_ROWS[(c + j) % 4]
        temperature[c + j] = TEMPERATURES[j % 2]
        if j < 10:
            density[c + j] = 0.
        elif j < 20:
            density[c + j] = DENSITIES[j % 4]
            heating[:, c + j] = data[row, 14:16] * 1.e-7 / o.PLANCK
        else:
            density[c + j] = 0.
            J[:, c + j] = data[row, :14]
            heating[:, c + j] = data[row, 14:16] * 1.e-7 / o.PLANCK
    x = np.zeros((o.NION, N))
    x[:2] = 1.e-6
    for a in (J, heating, density, temperature, variant, x):
        a.setflags(write=False)
    return SimpleNamespace(J=J, heating=heating, number_density=density,
                           temperature=temperature, x=x, variant=variant)


def oracle_simulation(crfac, J, heating):
    """The oracle's grid with the lattice's cells and the given integrals."""
    cell = cells()
    sim = o.OracleSimulation(NCELL, ANCHOR, SIDES)
    sim.set_sources([[0.5 * SIDES[0], 0.5 * SIDES[1], 0.]], [1.], LUMINOSITY)
    m = sim.model
    m.xsec_type = o.XSEC_VERNER
    m.recomb_type = o.RECOMB_VERNER
    for i, a in enumerate(ABUNDANCES):
        m.abundance[1 + i] = a
    m.do_temperature = 1
    m.t_min_iteration = MIN_ITERATION
    m.t_epsilon = EPSILON
    m.t_max_iterations = MAX_ITERATIONS
    m.pahfac = PAHFAC
    m.crfac = crfac
    m.crlim = CRLIM
    m.crscale = CRSCALE
    m.t_min_ionized = T_MIN_IONIZED
    sim.number_density[:] = cell.number_density
    sim.temperature[:] = cell.temperature
    sim.x[:] = cell.x
    sim.J[:] = J
    sim.heating[:] = heating
    return sim


def _result(sim):
    return SimpleNamespace(T=sim.temperature.copy(), x=sim.x.copy(),
                           heating=sim.heating.copy())


def _moved(a, b, tol):
    """|a - b| > tol |a| (a NaN on either side counts as moved)"""
    return ~(np.abs(a - b) <= tol * np.abs(a))


@functools.lru_cache(maxsize=None)
def solved(crfac):
    """The oracle's solution of the lattice for the model with the given cosmic
    ray factor: T[N], x[14][N], heating[2][N] (normalised), nsteps[N],
    branches[N] (oracle_lib.TB bits), ill[N] (ill-conditioned cells), and
    `untraced`, the same solve through cmio_update_cells."""
    cell = cells()
    sim = oracle_simulation(crfac, cell.J, cell.heating)
    nsteps, branches = sim.calculate_temperature_traced(TOTWEIGHT)
    out = _result(sim)
    sim = oracle_simulation(crfac, cell.J, cell.heating)
    sim.update(LOOP_TEMPERATURE, TOTWEIGHT)
    untraced = _result(sim)
    rng = np.random.default_rng(20240607)
    ill = np.zeros(N, dtype=bool)
    for _ in range(2):
        uJ = rng.uniform(-1., 1., cell.J.shape)
        uh = rng.uniform(-1., 1., cell.heating.shape)
        sim = oracle_simulation(
            crfac, cell.J * (1. + CONDITION_PERTURBATION * uJ),
            cell.heating * (1. + CONDITION_PERTURBATION * uh))
        steps, taken = sim.calculate_temperature_traced(TOTWEIGHT)
        ill |= _moved(out.T, sim.temperature, CONDITION_T)
        ill |= _moved(out.x, sim.x, CONDITION_X).any(axis=0)
        # a solve that wanders (the line cooling's level populations are
        # nearly singular around 6.5e5 K: the loss jumps by a factor 20 within
        # 0.2 % of T) can reach the same clamp - T > 1e10 K once the loss
        # touches 0 - after 14, 30 or 44 steps: same result, another path
        ill |= (steps != nsteps) | (taken != branches)
    out.nsteps, out.branches, out.ill, out.untraced = \
        nsteps, branches, ill, untraced
    for a in (out.T, out.x, out.heating, nsteps, branches, ill, untraced.T,
              untraced.x, untraced.heating):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ionized(crfac=0.):
    """The oracle's ionization balance (no temperature solve: a loop at the
    minimum iteration) of the lattice: x[14][N], and ill[N] by the recipe of
    solved() - the hydrogen / helium iteration stops at a relative change of
    1e-4 and its closed forms cancel for nearly neutral and nearly ionized
    cells - with a tenth of this check's tolerance of 1e-9 as the limit."""
    cell = cells()
    sim = oracle_simulation(crfac, cell.J, cell.heating)
    sim.update(LOOP_IONIZATION, TOTWEIGHT)
    out = _result(sim)
    rng = np.random.default_rng(20240608)
    out.ill = np.zeros(N, dtype=bool)
    for _ in range(2):
        uJ = rng.uniform(-1., 1., cell.J.shape)
        sim = oracle_simulation(
            crfac, cell.J * (1. + CONDITION_PERTURBATION * uJ), cell.heating)
        sim.update(LOOP_IONIZATION, TOTWEIGHT)
        moved = _moved(out.x, sim.x, CONDITION_X_IONIZATION)
        moved &= ~(np.isnan(out.x) & np.isnan(sim.x))
        out.ill |= moved.any(axis=0)
    # The iteration divides by 1 - h0 and multiplies by 1 - he0, and the
    # metals' charge transfer follows n (1 - h0): where one ulp of a fraction
    # just below 1 is a larger relative change of 1 - fraction than the
    # perturbation above, that perturbation says nothing about the cell
    ulp = np.finfo(np.float64).epsneg
    for fraction in out.x[:2]:
        rest = 1. - fraction
        out.ill |= (rest > 0.) & (ulp > CONDITION_PERTURBATION * rest)
    for a in (out.T, out.x, out.heating, out.ill):
        a.setflags(write=False)
    return out


def branch_counts(branches):
    """{branch name: number of cells that took it}"""
    return {name: int(np.count_nonzero(branches & bit))
            for name, bit in o.TB.items()}
