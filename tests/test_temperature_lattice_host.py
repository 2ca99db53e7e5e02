"""The lattice of tests/temperature_lattice.py on the oracle alone: it must
drive every branch of the temperature solve, stay well-conditioned and finite,
and the traced solve must be the untraced one. What the device makes of the
same cells is in test_gpu_temperature_branches.py."""
import ctypes as C

import numpy as np

import temperature_lattice as tl

MIN_CELLS_PER_BRANCH = 8
# arms of the solve the oracle reaches on no input tried (the lattice; 80000
# random cells from all rows of tbal_testdata.txt with J and heating scaled
# independently by 1e-20 .. 1e20, heating factors from -1e8 to 1e4, single J
# zeroed, densities 1 .. 1e12 m^-3, both models): gain1 <= 0 < gain2 needs the
# gain at 1.1 T to vanish while that at 0.9 T does not - the PAH and He
# Ly-alpha terms are positive whenever anything is ionized, and a negative
# photoheating large enough to cancel them does so at both temperatures
UNREACHED = ("GAIN_M99",)


def test_lattice_drives_every_branch(oracle):
    models = [tl.solved(0.), tl.solved(1.)]
    counts = [tl.branch_counts(s.branches) for s in models]
    print("cells per branch, crfac 0:", counts[0])
    print("cells per branch, crfac 1:", counts[1])
    for name in oracle.TEMPERATURE_BRANCHES:
        total = counts[0][name] + counts[1][name]
        if name in UNREACHED:
            continue
        assert total >= MIN_CELLS_PER_BRANCH, (name, total)
    # the cosmic ray branches belong to the model that has cosmic rays
    assert counts[0]["CRLIM"] == 0 and counts[0]["COSMIC_RAY_GAIN"] == 0
    assert counts[1]["CRLIM"] >= MIN_CELLS_PER_BRANCH
    assert counts[1]["COSMIC_RAY_GAIN"] >= MIN_CELLS_PER_BRANCH
    # ... in every z layer (each has its own exp(-|z| / crscale))
    layer = np.arange(tl.N) % 4
    for z in range(4):
        took = models[1].branches[layer == z] & oracle.TB["COSMIC_RAY_GAIN"]
        assert np.count_nonzero(took) >= MIN_CELLS_PER_BRANCH, z
    # cells that end at t_max_iterations: what temp_finish_kernel is for
    for s in models:
        ended = (s.branches & oracle.TB["MAX_ITERATIONS"]) != 0
        assert np.array_equal(ended & (s.nsteps == tl.MAX_ITERATIONS), ended)
    # the trace agrees with what it describes
    for s in models:
        b = s.branches
        neutral = (b & (oracle.TB["NO_RADIATION"] | oracle.TB["CRLIM"])) != 0
        assert np.array_equal(neutral, s.nsteps == 0)
        assert (s.T[neutral] == 500.).all()
        assert (s.T[(b & oracle.TB["CLIPPED"]) != 0] == 30000.).all()
        zeroed = (b & oracle.TB["METALS_ZEROED"]) != 0
        assert (s.x[2:, zeroed] == 0.).all()
        assert (s.x[0, (b & oracle.TB["JH_ZERO"]) != 0] == 1.).all()
        assert (s.x[1, (b & oracle.TB["JHE_ZERO"]) != 0] == 1.).all()


def test_lattice_is_well_conditioned_and_finite():
    for crfac in (0., 1.):
        s = tl.solved(crfac)
        share = np.count_nonzero(s.ill) / tl.N
        print("crfac %g: %d of %d cells ill-conditioned (%.2f %%)" % (
            crfac, np.count_nonzero(s.ill), tl.N, 100. * share))
        assert share <= tl.MAX_ILL_SHARE
        assert np.isfinite(s.T).all() and np.isfinite(s.x).all()
        assert np.isfinite(s.heating).all()
    both = np.count_nonzero(tl.solved(0.).ill) + \
        np.count_nonzero(tl.solved(1.).ill)
    assert both <= tl.MAX_ILL_SHARE * 2 * tl.N


def test_ionization_balance_keeps_its_special_cells():
    """the ionization-only balance of the lattice: what the oracle itself
    cannot pin down to a tenth of the check's tolerance is excused from the
    device check; every kind of cell that check is about stays in it"""
    cell = tl.cells()
    ion = tl.ionized(0.)
    well = ~ion.ill
    print("ionization balance: %d of %d cells ill-conditioned (%.2f %%)" % (
        np.count_nonzero(ion.ill), tl.N,
        100. * np.count_nonzero(ion.ill) / tl.N))
    special = cell.variant == -1
    kinds = {
        "J_H = 0": cell.variant == tl.VARIANTS.index("JH_zero"),
        "J_He = 0": cell.variant == tl.VARIANTS.index("JHe_zero"),
        "J(O0) = 0": cell.variant == tl.VARIANTS.index("JO0_zero"),
        "vacuum": special & (cell.number_density == 0.),
        "no radiation": special & (cell.J[0] == 0.) &
        (cell.number_density > 0.),
    }
    for name, kind in kinds.items():
        assert np.count_nonzero(kind & well) >= 8, name
    # a cell without hydrogen-ionizing radiation is neutral, whatever J_He
    dark = kinds["J_H = 0"] | kinds["no radiation"]
    assert (ion.x[:2, dark] == 1.).all()
    assert (ion.x[:, kinds["vacuum"]] == 0.).all()


def test_traced_solve_is_the_untraced_one(oracle):
    """grid level: cmio_calculate_temperature_range_traced against
    cmio_update_cells; cell level: cmio_temperature_cell_traced against
    cmio_temperature_cell."""
    L = oracle.lib()
    cell = tl.cells()
    for crfac in (0., 1.):
        s = tl.solved(crfac)
        assert np.array_equal(s.T, s.untraced.T)
        assert np.array_equal(s.x, s.untraced.x)
        assert np.array_equal(s.heating, s.untraced.heating)
        sim = tl.oracle_simulation(crfac, cell.J, cell.heating)
        for c in list(range(0, tl.N, 97)) + [tl.N - 1]:
            out = []
            for traced in (False, True):
                T = C.c_double(cell.temperature[c])
                J = np.ascontiguousarray(cell.J[:, c])
                # jfac is 1, so the grid's normalised heating is hfac x this
                h = np.ascontiguousarray(cell.heating[:, c])
                x = np.ascontiguousarray(cell.x[:, c])
                args = [C.byref(sim.model), 1., oracle.PLANCK,
                        cell.number_density[c], 0.3 * tl.CRSCALE, C.byref(T),
                        J.ctypes.data_as(oracle.dp),
                        h.ctypes.data_as(oracle.dp),
                        x.ctypes.data_as(oracle.dp)]
                if traced:
                    nsteps, taken = C.c_int32(-1), C.c_uint32(0xffffffff)
                    L.cmio_temperature_cell_traced(
                        *args, C.byref(nsteps), C.byref(taken))
                    assert 0 <= nsteps.value <= tl.MAX_ITERATIONS
                    assert taken.value < 1 << len(oracle.TEMPERATURE_BRANCHES)
                    assert (nsteps.value == 0) == bool(
                        taken.value & (oracle.TB["NO_RADIATION"] |
                                       oracle.TB["CRLIM"]))
                else:
                    L.cmio_temperature_cell(*args)
                out.append((T.value, x.tobytes(), h.tobytes()))
            assert out[0] == out[1], c
