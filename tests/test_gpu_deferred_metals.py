"""The hydrogen-only update of the whole grid in two halves - x[0], x[1], the
heating terms, the transport and the padded records in every iteration,
x[2..13] when somebody looks (`defer_metals=1`, `update_writes_pad=1`, the
defaults) - against an engine given the same calls with
`defer_metals=0 update_writes_pad=0` ("eager"): the same helpers on the same
values (the library is built with -ffp-contract=off: no contraction that
could differ between the two), so every reader must see the same 64-bit
patterns, whichever call of the engine it comes through and whatever happened
between the update and the look. Grids, temperatures and seeded state are
test_gpu_update_reuse.py's."""
import numpy as np
import pytest

from test_gpu_update_reuse import (SHAPES, TOTWEIGHT, make_engine, same_bits,
                                   state, temperatures)

pytestmark = pytest.mark.gpu

PATTERNS = ["uniform", "slabs_row_boundary", "slabs_mid_row", "every_cell",
            "one_cell_last_chunk"]
LINES = ["OI_6300", "NII_6584", "OIII_5007"]
# x[5] is what the issue of this change names; with no ionizing radiation of
# their own the metals' balance leaves it zero everywhere, which is also what
# upload_cells left: x[4] and x[7] (N0, O0: one in neutral gas, the charge
# transfer balance in ionized gas) tell a stale field from a settled one
LOOKED_AT = [5, 4, 7]


def E():
    from cmacionize_amd import engine
    return engine


# (no helium: a hydrogen-only run has no helium intensities for its balance)
METALS = [0., 2.2e-4, 4.e-5, 3.3e-4, 5.e-5, 9.e-6]


def pair(shape, track_heating=False, verner_rates=False, reuse=1):
    """(deferred, eager): two engines that differ in the two keys alone."""
    deferred = make_engine(shape, track_heating, verner_rates)
    eager = make_engine(shape, track_heating, verner_rates)
    for eng in (deferred, eager):
        eng.set_abundances(METALS)
    deferred.set_tuning(update_reuse=reuse)
    eager.set_tuning(update_reuse=reuse, defer_metals=0, update_writes_pad=0)
    return deferred, eager


def load(eng, density, T, J, heating=None):
    n = density.size
    x = np.zeros((14, n))
    x[0] = 1.e-6
    x[1] = 1.e-6
    eng.upload_cells(density, T, x)
    eng.upload_field(E().FIELD_MEAN_INTENSITY, J)
    if heating is not None:
        for k in range(2):
            eng.upload_field(E().FIELD_HEATING + k, heating[k])


def fractions(eng, ions=range(14)):
    return [eng.download_field(E().FIELD_IONIC_FRACTION + i) for i in ions]


def assert_same(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert same_bits(a, b), (k, int((a != b).sum()))


def start(shape, pattern="slabs_mid_row", **kw):
    """Both engines after one whole-grid update of the seeded state."""
    n = int(np.prod(shape))
    T = temperatures(pattern, n)
    J, heating, density = state(n)
    deferred, eager = pair(shape, **kw)
    for eng in (deferred, eager):
        load(eng, density, T, J, heating if kw.get("track_heating") else None)
        eng.update_cells(0, TOTWEIGHT)
    assert deferred.update_state()[0] and not eager.update_state()[0]
    return deferred, eager, (density, T, J)


@pytest.mark.parametrize("reuse", [0, 1])
@pytest.mark.parametrize("track_heating", [False, True])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_deferred_equals_eager(shape, pattern, track_heating, reuse):
    deferred, eager, (density, T, J) = start(
        shape, pattern, track_heating=track_heating, reuse=reuse)
    got, want = fractions(deferred), fractions(eager)
    assert not deferred.update_state()[0]
    if track_heating:
        for eng, out in ((deferred, got), (eager, want)):
            out += [eng.download_field(E().FIELD_HEATING + k)
                    for k in range(2)]
    deferred.close()
    eager.close()
    assert_same(got, want)
    # (the seeded state has every kind of cell: the comparison is not one of
    # zeros with zeros)
    ionized = (J > 0.) & (density > 0.)
    assert ionized.any() and (~ionized & (density > 0.)).any()
    assert (density == 0.).any()
    assert (want[4][~ionized & (density > 0.)] == 1.).all()  # N0
    assert (want[4][density == 0.] == 0.).all()


@pytest.mark.parametrize("reuse", [0, 1])
@pytest.mark.parametrize("pattern", ["uniform", "slabs_mid_row", "every_cell"])
def test_deferred_equals_eager_with_fitted_rates(pattern, reuse):
    """... with recombination rates that depend on the temperature (the
    Verner fits): here the metals' fractions of the ionized cells are not
    trivial."""
    deferred, eager, _ = start(SHAPES[1], pattern, track_heating=True,
                               verner_rates=True, reuse=reuse)
    got, want = fractions(deferred), fractions(eager)
    for eng, out in ((deferred, got), (eager, want)):
        out += [eng.download_field(E().FIELD_HEATING + k) for k in range(2)]
    deferred.close()
    eager.close()
    assert_same(got, want)
    assert any(((w > 0.) & (w < 1.)).any() for w in want[2:14])


@pytest.mark.parametrize("trigger", ["download", "emissivities", "tensor"])
def test_every_trigger_settles(trigger):
    deferred, eager, _ = start(SHAPES[1], verner_rates=True)
    out = []
    for eng in (deferred, eager):
        if trigger == "download":
            out.append(fractions(eng, LOOKED_AT))
        elif trigger == "emissivities":
            em = eng.compute_emissivities(LINES)
            out.append([em[name] for name in LINES])
        else:
            t = eng.field_tensor(E().FIELD_IONIC_FRACTION + 7)
            eng.synchronize()
            out.append([t.cpu().numpy().copy()])
    assert not deferred.update_state()[0]
    deferred.close()
    eager.close()
    assert_same(*out)
    if trigger != "emissivities":
        assert (out[1][-1] != 0.).any()


@pytest.mark.parametrize("field", ["temperature", "x0", "density"])
def test_mutation_order(field):
    """An upload between the update and the look: the fractions are those of
    the state the update saw."""
    deferred, eager, (density, T, J) = start(SHAPES[1], verner_rates=True)
    before = fractions(eager, LOOKED_AT)
    rng = np.random.default_rng(3)
    for eng in (deferred, eager):
        if field == "temperature":
            eng.upload_field(E().FIELD_TEMPERATURE, T * 1.7)
        elif field == "x0":
            eng.upload_field(E().FIELD_IONIC_FRACTION, rng.random(T.size))
        else:
            eng.upload_field(E().FIELD_NUMBER_DENSITY,
                             np.where(density > 0., 0., 3.e8))
    got, want = fractions(deferred, LOOKED_AT), fractions(eager, LOOKED_AT)
    deferred.close()
    eager.close()
    assert_same(got, want)
    assert_same(want, before)
    assert (want[1] != 0.).any()


def test_replacement():
    """Two whole-grid updates without a look between them: the second
    replaces what the first left pending."""
    shape = SHAPES[0]
    n = int(np.prod(shape))
    deferred, eager, (density, T, J) = start(shape, verner_rates=True)
    J2 = np.roll(J, 777) * 3.
    for eng in (deferred, eager):
        eng.upload_field(E().FIELD_MEAN_INTENSITY, J2)
        eng.update_cells(1, TOTWEIGHT)
    assert deferred.update_state()[0]
    got, want = fractions(deferred), fractions(eager)
    deferred.close()
    eager.close()
    assert_same(got, want)
    assert n == J2.size


def test_pending_across_an_iteration():
    """reset_grid and shoot neither need nor disturb the pending fractions; J
    is gone by the time they are made, so this is the gate bits' test."""
    deferred, eager, _ = start(SHAPES[0], verner_rates=True)
    want = fractions(eager, range(2, 14))
    deferred.reset_grid()
    deferred.shoot(42, 1, 0, 20000)
    deferred.synchronize()
    assert deferred.update_state()[0]
    got = fractions(deferred, range(2, 14))
    deferred.close()
    eager.close()
    assert_same(got, want)


def test_ranges():
    """A partial update after a deferred one: first what is pending, then its
    own cells."""
    shape = SHAPES[1]
    n = int(np.prod(shape))
    deferred, eager, (density, T, J) = start(shape, verner_rates=True)
    J2 = np.roll(J, 123) * 0.5
    for eng in (deferred, eager):
        eng.upload_field(E().FIELD_MEAN_INTENSITY, J2)
        eng.update_cells_range(1, TOTWEIGHT, n // 3, n // 3)
    assert not deferred.update_state()[0]
    got, want = fractions(deferred), fractions(eager)
    deferred.close()
    eager.close()
    assert_same(got, want)


def transport_step(eng, n_packets=100003):
    eng.reset_grid()
    eng.shoot(11, 2, 5, n_packets)
    tw, tc, ns = eng.get_counters()
    return tw, tc, ns, eng.download_field(E().FIELD_MEAN_INTENSITY)


@pytest.mark.parametrize("between", ["nothing", "density", "range"])
@pytest.mark.parametrize("shape", SHAPES)
def test_padded_records(shape, between):
    """The padded records written by the update against those written by
    pad_record_kernel, read by the padded march: the same counters, J_H at
    the bound test_gpu_bundle_order.py has for a changed order of adds.
    `between`: something that writes transport records after the update - the
    update's padded records must not be used then."""
    n = int(np.prod(shape))
    T = temperatures("uniform", n)
    J, _, density = state(n)
    out = []
    for writes_pad in (1, 0):
        eng = make_engine(shape, False)
        eng.set_tuning(update_writes_pad=writes_pad, pad_march=1)
        load(eng, density, T, J)
        # (a first transport step: the padded records with their ghost layer)
        transport_step(eng, 1000)
        assert eng.update_state()[1]
        eng.upload_field(E().FIELD_MEAN_INTENSITY, J)
        eng.update_cells(0, TOTWEIGHT)
        assert eng.update_state()[1] == bool(writes_pad)
        if between == "density":
            moved = np.roll(density, 1000)
            eng.upload_field(E().FIELD_NUMBER_DENSITY, moved)
            assert not eng.update_state()[1]
        elif between == "range":
            eng.upload_field(E().FIELD_MEAN_INTENSITY, np.roll(J, 99))
            eng.update_cells_range(1, TOTWEIGHT, n // 3, n // 3)
            assert not eng.update_state()[1]
        out.append(transport_step(eng))
        eng.close()
    (tw, tc, ns, JH), (tw0, tc0, ns0, JH0) = out
    assert tw == tw0 and np.array_equal(tc, tc0) and ns == ns0 and ns > 0
    assert np.allclose(JH, JH0, rtol=1e-11, atol=1e-13 * np.abs(JH0).max())
    assert JH0.max() > 0.


def test_pointer_escape():
    """A pointer to x[3] in the caller's hands: that engine defers no more;
    another that never asked does; both hold the same fractions."""
    shape = SHAPES[1]
    n = int(np.prod(shape))
    T = temperatures("slabs_mid_row", n)
    J, _, density = state(n)
    asked = make_engine(shape, False, True)
    never = make_engine(shape, False, True)
    for eng in (asked, never):
        load(eng, density, T, J)
        eng.update_cells(0, TOTWEIGHT)
    view = asked.field_tensor(E().FIELD_IONIC_FRACTION + 3)
    assert asked.update_state()[0] is False
    assert asked.update_state()[2] is False and never.update_state()[2] is True
    for eng in (asked, never):
        eng.upload_field(E().FIELD_MEAN_INTENSITY, J * 2.)
        eng.update_cells(1, TOTWEIGHT)
    assert not asked.update_state()[0] and never.update_state()[0]
    asked.synchronize()
    through_view = view.cpu().numpy().copy()
    got, want = fractions(asked), fractions(never)
    asked.close()
    never.close()
    assert_same(got, want)
    assert same_bits(through_view, want[3])
