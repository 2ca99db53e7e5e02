"""GPU tests of how the first generation's bundles are composed (tuning key
class_order: the tau classes of every second coarse direction bin the other
way round). The key moves a packet's place in the launch's order and nothing
else - ids, random numbers and emission rows stay - so against the static
split with every scheduling key off the packet counters and the DDA step
count are exactly equal and the integrals differ by the order of the atomic
adds only (the tolerance of test_gpu_span_schedule.py). Below 2^22 packets the
engine uses no tau classes: sort_tau_bits is forced to 1, 2 and 3.

The last test checks the effect itself: fewer trips of the waves through the
march loop for the same DDA steps."""
import numpy as np
import pytest

from test_gpu_transport import make_engine

pytestmark = pytest.mark.gpu

# one wave's chunk is 64 positions, a block's span 8 chunks = 512; a coarse
# direction bin holds 64 x 2^sort_tau_bits packets or more, so the first bins of
# odd index appear at 256 (1 bit), 512 (2 bits) and 1024 packets (3 bits): below,
# at and above one chunk, one span, one and a half and two spans, several spans
COUNTS = [1, 63, 64, 65, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025,
          4097, 100003]
# 586 spans, the last short, for at most one block per CU
MANY_SPANS = 300003
TAU_BITS = [1, 2, 3]

OFF = dict(span_claim=0, emit_before_flush=0, xcd_remap=0, class_order=0,
           sort_tau_bits=-1, max_packets_per_launch=1 << 27, park_in_place=1,
           max_blocks_per_cu=8)
# the schedules the orders are flown with: the claimed spans with the early
# refill (the defaults), with one cursor per XCD, and the static split
SCHEDULES = [dict(span_claim=1, emit_before_flush=1, xcd_remap=0),
             dict(span_claim=1, emit_before_flush=1, xcd_remap=1),
             dict(span_claim=0, emit_before_flush=0, xcd_remap=0)]

_engines = {}
_reference = {}


def engine(kind):
    """One engine per set-up, shared by the module's tests."""
    if kind in _engines:
        return _engines[kind]
    if kind == "plain16":
        eng = make_engine(16, track_heating=False)
    elif kind == "plain24":
        eng = make_engine(24, track_heating=False)
    elif kind == "heating24":
        eng = make_engine(24, track_heating=True)
    elif kind == "reemission16":
        eng = make_engine(16, track_heating=False)
        eng.set_reemission(1)
    elif kind == "uniform32":
        # a fixed neutral fraction: optical depth 4.9 from the star to the
        # faces of the box, so the flights of the 8 classes end between the
        # first cells and the faces
        eng = make_engine(32, track_heating=False, xH=5.e-4)
    elif kind == "block24":
        # the middle block of 3 x 1 x 1 (it holds the star): it flies its
        # selection of every launch's packets and hands flights over
        from cmacionize_amd import STROMGREN as S
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


def shoot(kind, n, **tuning):
    from cmacionize_amd import engine as E
    eng = engine(kind)
    settings = dict(OFF)
    settings.update(tuning)
    eng.set_tuning(**settings)
    eng.reset_grid()
    if kind == "block24":
        eng.reset_exports()
    eng.shoot(11, 2, 5, n)
    tw, tc, ns = eng.get_counters()
    out = dict(tw=tw, tc=tc, ns=ns, wave_steps=eng.get_wave_steps(),
               J=eng.download_field(E.FIELD_MEAN_INTENSITY))
    if kind == "heating24":
        out["heating"] = eng.download_field(E.FIELD_HEATING)
    if kind == "block24":
        out["exports"] = eng.get_export_count()
    return out


def reference(kind, n):
    """The static split with every scheduling key off, once per set-up and
    count."""
    if (kind, n) not in _reference:
        _reference[(kind, n)] = shoot(kind, n)
    return _reference[(kind, n)]


def check_same(got, ref, n=None):
    if n is not None:
        assert ref["tw"] == n
    assert got["tw"] == ref["tw"]
    assert np.array_equal(got["tc"], ref["tc"])
    assert got["ns"] == ref["ns"]
    for field in ("J", "heating"):
        if field in ref:
            a, b = got[field], ref[field]
            assert np.allclose(a, b, rtol=1e-11, atol=1e-13 * np.abs(b).max())
    assert ref["J"].max() > 0. or ref["ns"] == 0
    if "exports" in ref:
        assert got["exports"] == ref["exports"]


def check_orders(kind, n, tau_bits, schedules=SCHEDULES, **tuning):
    """Both class orders with each schedule against the reference."""
    ref = reference(kind, n)
    for schedule in schedules:
        for class_order in (0, 1):
            settings = dict(schedule)
            settings.update(tuning)
            check_same(shoot(kind, n, class_order=class_order,
                             sort_tau_bits=tau_bits, **settings),
                       ref, None if kind == "block24" else n)
    return ref


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("tau_bits", TAU_BITS)
@pytest.mark.parametrize("kind", ["plain16", "plain24"])
def test_class_order_equals_the_static_split(kind, tau_bits, n):
    check_orders(kind, n, tau_bits)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("tau_bits", TAU_BITS)
def test_class_order_over_several_launches(tau_bits, n):
    """Every launch of a call has its own bins (1024 is the least a launch
    can be limited to)."""
    check_orders("plain24", n, tau_bits, max_packets_per_launch=1024)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("tau_bits", TAU_BITS)
def test_class_order_with_heating(tau_bits, n):
    check_orders("heating24", n, tau_bits)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("tau_bits", TAU_BITS)
def test_class_order_with_reemission(tau_bits, n):
    """The first generation parks absorbed packets at their positions in the
    launch's order - the order that moves - or through the queue's counter."""
    check_orders("reemission16", n, tau_bits)
    check_orders("reemission16", n, tau_bits, schedules=SCHEDULES[:1],
                 park_in_place=0)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("tau_bits", TAU_BITS)
def test_class_order_on_a_block_of_a_decomposed_grid(tau_bits, n):
    """A selection of the launch's packets is ordered and flies; flights leave
    the block."""
    ref = check_orders("block24", n, tau_bits)
    check_orders("block24", n, tau_bits, schedules=SCHEDULES[:1],
                 max_packets_per_launch=1024)
    if n >= 4097:
        assert ref["exports"] > 0 and ref["ns"] > 0


@pytest.mark.parametrize("tau_bits", TAU_BITS)
@pytest.mark.parametrize("kind", ["plain24", "heating24", "reemission16",
                                  "block24"])
def test_class_order_with_blocks_that_take_many_spans(kind, tau_bits):
    """One block per CU and more than twice as many spans: every block takes
    span after span through bin after bin and, with xcd_remap, moves on to the
    next XCD's cursor."""
    check_orders(kind, MANY_SPANS, tau_bits, schedules=SCHEDULES[:2],
                 max_blocks_per_cu=1)


@pytest.mark.parametrize("n", [513, 1500])
def test_class_order_matches_oracle(oracle, n):
    """Two and three spans, the last short; with one class bit these launches
    have four and eight coarse bins."""
    sim = oracle.stromgren_simulation(16)
    sim.reset()
    sim.totweight = 0.
    sim.typecount[:] = 0.
    sim.shoot(11, 2, 5, n)
    for schedule in SCHEDULES:
        got = shoot("plain16", n, class_order=1, sort_tau_bits=1, **schedule)
        assert got["tw"] == sim.totweight == n
        assert np.array_equal(got["tc"], sim.typecount)
        assert np.allclose(got["J"], sim.J[0], rtol=1e-9,
                           atol=1e-12 * sim.J[0].max())


def test_serpentine_classes_shorten_the_march():
    """Uniform 32^3 grid, 2e5 packets, 8 classes: 256 coarse bins of about 781
    packets, 12.2 chunks each, as in the headline run. With whole-bundle
    refills a bundle's trips through the march loop are its longest lane's
    steps, whatever block flies it: the count is exact, and the serpentine
    order must need fewer trips for the same DDA steps."""
    n = 200000
    schedule = dict(span_claim=1, emit_before_flush=1, sort_tau_bits=3)
    plain = shoot("uniform32", n, class_order=0, **schedule)
    serpentine = shoot("uniform32", n, class_order=1, **schedule)
    check_same(serpentine, plain, n)
    print("wave steps: class_order=0 %d, class_order=1 %d, ratio %.4f; "
          "lanes stepping per trip %.2f -> %.2f"
          % (plain["wave_steps"], serpentine["wave_steps"],
             serpentine["wave_steps"] / plain["wave_steps"],
             plain["ns"] / plain["wave_steps"],
             serpentine["ns"] / serpentine["wave_steps"]))
    assert plain["wave_steps"] > 0
    assert serpentine["wave_steps"] < plain["wave_steps"]
    # the same order flown by the static split takes the same trips
    static = shoot("uniform32", n, class_order=1, sort_tau_bits=3)
    assert static["wave_steps"] == serpentine["wave_steps"]

