"""GPU tests of what the padded hydrogen-only march reads and adds: records
that hold sigma_H n x_H (the cross section folded in once per cell, not once
per crossing) and, where every packet of a call carries one weight, table
sums of path lengths that are weighed where they leave the table.

The references are two paths of the same library that never read the padded
records: the block table on the transport records (`pad_march=0`) and a plain
atomic add per step (`aggregate=0`). The records' product is the one the march
formed, so which packet ends where cannot change: total weight, the four type
counts and the DDA step count are EXACTLY equal; J_H and the heating integral
are sums of positive terms in another order, or a weighed sum instead of a sum
of weighed terms: relative 1e-11 per cell, no absolute term. (Largest seen:
8.1e-12, the same figure at 64 and 65 packets on the 16^3 grid with and
without the heating term and with either build, so it is one packet's one
crossing and neither the records nor the weighing; presumably a very short
path, whose length is a difference of two wall parameters. Every other case
agrees to 5e-13 or better.)"""
import numpy as np
import pytest

from test_gpu_transport import make_engine

pytestmark = pytest.mark.gpu

# one wave's chunk is 64 positions: below, at and above it, several spans of
# 512, many blocks
COUNTS = [1, 63, 64, 65, 4097, 100003]
SHAPE24 = (24, 16, 20)
# FirstBuild of the plan: the padded march in its smaller blocks
FIRST_PAD = 2

BASE = dict(pad_march=1, pad_uniform=1, aggregate=2, sort_packets=1,
            span_claim=1, emit_before_flush=1, xcd_remap=0,
            max_packets_per_launch=1 << 27, park_in_place=1,
            update_writes_pad=1)
REFERENCES = [dict(pad_march=0), dict(aggregate=0, sort_packets=0)]

_engines = {}
_reference = {}


def fixed_rates(eng, sigma_H=None):
    from cmacionize_amd import STROMGREN as S
    sigma = np.zeros(14)
    sigma[0] = S["sigma_H"] if sigma_H is None else sigma_H
    alpha = np.zeros(14)
    alpha[0] = S["alpha_H"]
    eng.set_cross_sections_fixed(sigma)
    eng.set_recombination_rates_fixed(alpha)


def noncubic_engine(heat):
    """24 x 16 x 20 cells of different sides, a star off the centre and off
    the cell walls, a slab of vacuum and a neutral clump: three padded
    strides, ghost cells behind every face, vacuum records."""
    from cmacionize_amd import GpuEngine, STROMGREN as S
    pc = 3.086e16
    shape = SHAPE24
    n = int(np.prod(shape))
    eng = GpuEngine(shape, (-4. * pc, -2. * pc, -3. * pc),
                    (9. * pc, 5. * pc, 7. * pc), (0, 0, 0), device=0,
                    track_heating=heat)
    eng.set_sources([[0.37 * pc, 0.21 * pc, -0.43 * pc]], [1.],
                    S["luminosity"])
    eng.set_spectrum_monochromatic(1.2 * S["frequency"])
    fixed_rates(eng)
    dens = np.full(shape, S["density"])
    dens[17:19] = 0.
    xH = np.full(shape, 1.e-4)
    xH[3:6, 2:5, 9:13] = 1.
    x = np.zeros((14, n))
    x[0] = xH.ravel()
    x[1] = S["xHe"]
    eng.upload_cells(dens.ravel(), np.full(n, S["temperature"]), x)
    return eng


def engine(kind):
    """One engine per set-up, shared by the module's tests."""
    from cmacionize_amd import STROMGREN as S
    from cmacionize_amd import engine as E
    if kind in _engines:
        return _engines[kind]
    if kind == "plain16":
        eng = make_engine(16, track_heating=False)
    elif kind == "heating16":
        eng = make_engine(16, track_heating=True)
    elif kind == "plain24":
        eng = noncubic_engine(False)
    elif kind == "heating24":
        eng = noncubic_engine(True)
    elif kind == "twostars16":
        # two discrete sources of equal weight: one photon weight
        eng = make_engine(16, track_heating=False)
        side = S["sides"][0]
        eng.set_sources([[0.21 * side, -0.13 * side, 0.07 * side],
                         [-0.17 * side, 0.09 * side, -0.23 * side]],
                        [0.5, 0.5], S["luminosity"])
    elif kind == "mixed16":
        # a star and a continuous source of 2.5 times its luminosity, half of
        # the packets each: the continuous source's carry the weight 2.5
        eng = make_engine(16, track_heating=False)
        eng.set_continuous_spectrum_monochromatic(1.1 * S["frequency"])
        eng.set_continuous_source(E.CONTINUOUS_ISOTROPIC,
                                  2.5 * S["luminosity"])
    elif kind == "reemission16":
        eng = make_engine(16, track_heating=False)
        eng.set_reemission(1)
    elif kind == "block24":
        # the middle block of 3 x 1 x 1 (it holds the star): it flies its
        # selection of every launch's packets and hands flights over
        from cmacionize_amd.simulation import (DomainDecomposition,
                                               DomainGpuBackend)
        from test_gpu_domain import configure
        dec = DomainDecomposition((24,) * 3, (3, 1, 1))
        backend = DomainGpuBackend(dec, 1, S["anchor"], S["sides"], device=0,
                                   track_heating=False,
                                   export_capacity=1 << 19)
        configure(backend.engine, "stromgren",
                  int(np.prod(dec.block(1)[1])))
        _engines[kind] = backend.engine
        _engines[kind + ":backend"] = backend  # owns the export buffer
        return backend.engine
    else:
        raise KeyError(kind)
    _engines[kind] = eng
    return eng


@pytest.fixture(scope="module", autouse=True)
def close_engines():
    yield
    for key, eng in _engines.items():
        if not key.endswith(":backend"):
            eng.close()
    _engines.clear()
    _reference.clear()


def result(eng, n, exports=False):
    from cmacionize_amd import engine as E
    eng.reset_grid()
    if exports:
        eng.reset_exports()
    eng.shoot(11, 2, 5, n)
    tw, tc, ns = eng.get_counters()
    out = dict(tw=tw, tc=tc, ns=ns, plan=eng.transport_plan(),
               J=eng.download_field(E.FIELD_MEAN_INTENSITY))
    if eng.track_heating_for_tests:
        out["heating"] = eng.download_field(E.FIELD_HEATING)
    if exports:
        out["exports"] = eng.get_export_count()
    return out


def shoot(kind, n, **tuning):
    eng = engine(kind)
    eng.track_heating_for_tests = kind.startswith("heating")
    settings = dict(BASE)
    settings.update(tuning)
    eng.set_tuning(**settings)
    return result(eng, n, exports=kind == "block24")


def references(kind, n):
    """Both reference paths, once per set-up and count; left unchanged."""
    if (kind, n) not in _reference:
        refs = [shoot(kind, n, **kw) for kw in REFERENCES]
        for ref in refs:
            assert ref["plan"][0] != FIRST_PAD and not ref["plan"][1]
        _reference[(kind, n)] = refs
    return _reference[(kind, n)]


def check_same(got, ref, n=None):
    if n is not None:
        assert ref["tw"] == n
    print("tw", got["tw"], ref["tw"], "tc", got["tc"], ref["tc"], "ns",
          got["ns"], ref["ns"])
    assert got["tw"] == ref["tw"]
    assert np.array_equal(got["tc"], ref["tc"])
    assert got["ns"] == ref["ns"]
    for field in ("J", "heating"):
        if field in ref:
            a, b = got[field], ref[field]
            nz = b != 0.
            print(field, "max relative difference",
                  np.abs(a[nz] / b[nz] - 1.).max() if nz.any() else 0.)
            assert np.allclose(a, b, rtol=1e-11, atol=0.)
    assert ref["J"].max() > 0. or ref["ns"] == 0
    if "exports" in ref:
        assert got["exports"] == ref["exports"]


def check_against_references(kind, n, uniform, total=True, **tuning):
    got = shoot(kind, n, **tuning)
    assert got["plan"] == (FIRST_PAD, uniform)
    for ref in references(kind, n):
        check_same(got, ref, n if total else None)
    return got


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", ["plain16", "plain24", "heating16",
                                  "heating24"])
def test_default_path_against_both_references(kind, n):
    """Heating off: the build for packets of one weight; on: a product per
    lane and step."""
    got = check_against_references(kind, n, not kind.startswith("heating"))
    if kind.endswith("24") and n >= 4097:
        J = got["J"].reshape(SHAPE24)
        assert not J[17:19].any()   # nothing tallied in vacuum
        assert J[19:].any()         # but packets cross it


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", ["plain24", "heating24"])
def test_per_lane_products_where_the_uniform_build_is_switched_off(kind, n):
    check_against_references(kind, n, False, pad_uniform=0)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("span_claim", [0, 1])
@pytest.mark.parametrize("kind", ["plain24", "heating16"])
def test_static_split_and_claimed_spans(kind, span_claim, n):
    check_against_references(kind, n, kind == "plain24",
                             span_claim=span_claim, emit_before_flush=0,
                             xcd_remap=span_claim)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", ["plain16", "heating24"])
def test_several_launches_in_one_call(kind, n):
    """(1024 is the least a launch can be limited to)"""
    check_against_references(kind, n, kind == "plain16",
                             max_packets_per_launch=1024)


@pytest.mark.parametrize("n", COUNTS)
def test_two_sources_of_equal_weight_take_the_uniform_build(n):
    check_against_references("twostars16", n, True)


@pytest.mark.parametrize("n", COUNTS)
def test_a_continuous_source_of_another_weight_takes_per_lane_products(n):
    # (half of the packets carry the weight 2.5: the total is not n)
    got = check_against_references("mixed16", n, False, total=False)
    if n >= 63:
        assert got["tw"] > n


@pytest.mark.parametrize("n", COUNTS)
def test_reemission_with_parking(n):
    """The first generation parks absorbed packets at their positions; the
    later generations never read the padded records."""
    check_against_references("reemission16", n, True)
    check_against_references("reemission16", n, True, park_in_place=0)


@pytest.mark.parametrize("n", COUNTS)
def test_block_of_a_decomposed_grid(n):
    """A selection of the launch's packets flies; flights leave the block:
    the selection (total weight, counts) and the hand-over count are equal."""
    got = check_against_references("block24", n, True, total=False)
    if n >= 4097:
        assert got["exports"] > 0 and got["ns"] > 0


def test_another_cross_section_between_two_shoots():
    """The records hold the cross section: a second shoot after
    cmi_gpu_set_cross_sections_fixed with another value must read records of
    that value - it equals a fresh engine's with it."""
    from cmacionize_amd import STROMGREN as S
    n = 100003
    other = 0.37 * S["sigma_H"]
    eng = make_engine(16, track_heating=False)
    eng.track_heating_for_tests = False
    eng.set_tuning(**BASE)
    first = result(eng, n)
    assert eng.update_state()[1]
    fixed_rates(eng, other)
    assert not eng.update_state()[1]
    second = result(eng, n)
    eng.close()
    fresh_engine = make_engine(16, track_heating=False)
    fresh_engine.track_heating_for_tests = False
    fixed_rates(fresh_engine, other)
    fresh_engine.set_tuning(**BASE)
    fresh = result(fresh_engine, n)
    fresh_engine.set_tuning(**dict(BASE, pad_march=0))
    plain = result(fresh_engine, n)
    fresh_engine.close()
    assert second["plan"] == fresh["plan"] == (FIRST_PAD, True)
    check_same(second, fresh, n)
    check_same(second, plain, n)
    # (and the cross section matters: fewer crossings end a flight)
    assert first["ns"] != second["ns"]


@pytest.mark.parametrize("between", ["nothing", "upload"])
def test_update_between_two_shoots(between):
    """The update writes the padded records itself (update_writes_pad=1) or
    leaves them to the next shoot: equal results - also with an upload of the
    density between update and shoot, after which the update's records must
    not be used."""
    from cmacionize_amd import engine as E
    n = 100003
    out = []
    for writes_pad in (1, 0):
        eng = noncubic_engine(False)
        eng.track_heating_for_tests = False
        eng.set_tuning(**dict(BASE, update_writes_pad=writes_pad))
        first = result(eng, n)
        assert eng.update_state()[1]
        # (the same integrals for both engines: J_H of a shoot varies with the
        # order of its atomic adds)
        if not out:
            J = first["J"]
        eng.upload_field(E.FIELD_MEAN_INTENSITY, J)
        eng.update_cells(0, float(n))
        assert eng.update_state()[1] == bool(writes_pad)
        if between == "upload":
            dens = eng.download_field(E.FIELD_NUMBER_DENSITY)
            eng.upload_field(E.FIELD_NUMBER_DENSITY,
                             np.roll(dens.reshape(SHAPE24), 3, axis=0))
            assert not eng.update_state()[1]
        second = result(eng, n)
        assert second["plan"] == (FIRST_PAD, True)
        eng.set_tuning(pad_march=0)
        check_same(second, result(eng, n), n)
        assert second["ns"] != first["ns"]
        out.append(second)
        eng.close()
    check_same(out[0], out[1], n)


def test_default_path_against_the_oracle(oracle):
    n = 100003
    sim = oracle.stromgren_simulation(16)
    sim.reset()
    sim.totweight = 0.
    sim.typecount[:] = 0.
    sim.shoot(11, 2, 5, n)
    got = shoot("plain16", n)
    assert got["plan"] == (FIRST_PAD, True)
    assert got["tw"] == sim.totweight == n
    assert np.array_equal(got["tc"], sim.typecount)
    # (the oracle marches with the reference's per-step arithmetic, the
    # engine incrementally: the bound of test_gpu_span_schedule.py's oracle
    # test)
    assert np.allclose(got["J"], sim.J[0], rtol=1e-9,
                       atol=1e-12 * sim.J[0].max())
