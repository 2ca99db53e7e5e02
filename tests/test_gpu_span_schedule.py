"""GPU tests of how the hydrogen-only table kernels schedule their bundles
(tuning keys span_claim, emit_before_flush): neither
changes which packet flies with which random numbers, so the packet counters
and the DDA step count are exactly those of the static split and the
integrals differ by the order of the atomic adds only (the tolerance of
test_gpu_transport.py::test_tuning_does_not_change_results)."""
import numpy as np
import pytest

from test_gpu_transport import make_engine

pytestmark = pytest.mark.gpu

# one wave's chunk is 64 positions, a block's span 8 chunks = 512: below,
# at and above one chunk and one span, several spans. (A launch has as many
# blocks as spans up to the device's limit: at these counts a block flies one
# span, or - another block was faster - two or none; MANY_SPANS below is the
# case where every block must take span after span.)
COUNTS = [1, 63, 64, 65, 511, 512, 513, 4097, 100003]
# 586 spans, the last short, for at most one block per CU
MANY_SPANS = 300003

OFF = dict(span_claim=0, emit_before_flush=0, xcd_remap=0,
           max_packets_per_launch=1 << 27, park_in_place=1,
           max_blocks_per_cu=8)

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
    out = dict(tw=tw, tc=tc, ns=ns,
               J=eng.download_field(E.FIELD_MEAN_INTENSITY))
    if kind == "heating24":
        out["heating"] = eng.download_field(E.FIELD_HEATING)
    if kind == "block24":
        out["exports"] = eng.get_export_count()
    return out


def reference(kind, n):
    """The static split with everything off, once per set-up and count."""
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


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("xcd_remap", [1, 0])
def test_claimed_spans_equal_the_static_split(n, xcd_remap):
    check_same(shoot("plain16", n, span_claim=1, xcd_remap=xcd_remap),
               reference("plain16", n), n)


@pytest.mark.parametrize("n", COUNTS)
def test_claimed_spans_over_several_launches(n):
    """The cursors start again in every launch of a call (1024 is the least
    a launch can be limited to)."""
    check_same(shoot("plain24", n, span_claim=1, xcd_remap=1,
                     max_packets_per_launch=1024),
               reference("plain24", n), n)


@pytest.mark.parametrize("n", COUNTS)
def test_claimed_spans_with_heating(n):
    check_same(shoot("heating24", n, span_claim=1, xcd_remap=1),
               reference("heating24", n), n)


@pytest.mark.parametrize("n", COUNTS)
def test_claimed_spans_with_reemission(n):
    """The first generation parks absorbed packets at their positions."""
    check_same(shoot("reemission16", n, span_claim=1, xcd_remap=1),
               reference("reemission16", n), n)
    check_same(shoot("reemission16", n, span_claim=1, park_in_place=0),
               reference("reemission16", n), n)


@pytest.mark.parametrize("n", COUNTS)
def test_claimed_spans_on_a_block_of_a_decomposed_grid(n):
    """A selection of the launch's packets flies; flights leave the block."""
    ref = reference("block24", n)
    check_same(shoot("block24", n, span_claim=1, xcd_remap=1), ref)
    check_same(shoot("block24", n, span_claim=1, xcd_remap=0,
                     max_packets_per_launch=1024), ref)
    if n >= 4097:
        assert ref["exports"] > 0 and ref["ns"] > 0


@pytest.mark.parametrize("emit_before_flush", [0, 1])
@pytest.mark.parametrize("xcd_remap", [0, 1])
@pytest.mark.parametrize("kind", ["plain24", "heating24", "reemission16",
                                  "block24"])
def test_blocks_that_take_many_spans(kind, xcd_remap, emit_before_flush):
    """One block per CU and more than twice as many spans: every block
    claims, flies and claims again; with xcd_remap the 8 parts of the spans
    do not divide evenly among the blocks of the 8 XCDs, so blocks go on with
    the next XCD's cursor. (A block of the decomposed grid flies a third of
    the packets: fewer spans per block.)"""
    n = MANY_SPANS
    check_same(shoot(kind, n, span_claim=1, xcd_remap=xcd_remap,
                     emit_before_flush=emit_before_flush,
                     max_blocks_per_cu=1),
               reference(kind, n), None if kind == "block24" else n)


@pytest.mark.parametrize("span_claim", [0, 1])
@pytest.mark.parametrize("kind", ["plain16", "heating24", "reemission16",
                                  "block24"])
def test_refill_ahead_of_the_flush_point(kind, span_claim):
    for n in (100003, 4097, 513, 65):
        check_same(shoot(kind, n, span_claim=span_claim,
                         emit_before_flush=1, xcd_remap=span_claim),
                   reference(kind, n), None if kind == "block24" else n)


@pytest.mark.parametrize("n", [65, 513, 1500])
@pytest.mark.parametrize("emit_before_flush", [0, 1])
def test_waves_and_blocks_without_positions_match_oracle(oracle, n,
                                                         emit_before_flush):
    """65 packets: two chunks for a block of eight waves, six waves without
    positions. 513 and 1500: two and three spans, the last short (one and
    eight chunks' worth missing), for as many blocks; a block that comes late
    may find every span taken and leaves at its first flush point."""
    sim = oracle.stromgren_simulation(16)
    sim.reset()
    sim.totweight = 0.
    sim.typecount[:] = 0.
    sim.shoot(11, 2, 5, n)
    for xcd_remap in (0, 1):
        got = shoot("plain16", n, span_claim=1, xcd_remap=xcd_remap,
                    emit_before_flush=emit_before_flush)
        assert got["tw"] == sim.totweight == n
        assert np.array_equal(got["tc"], sim.typecount)
        assert np.allclose(got["J"], sim.J[0], rtol=1e-9,
                           atol=1e-12 * sim.J[0].max())
