"""GPU tests of the bundle build of the padded first generation (tuning key
bundle_march) and of the width of the key's class groups (class_group_chunks).

The bundle build is the padded march's kernel made for launches in which every
refill fills a whole idle wave from one claimed chunk of 64: it emits every
packet with the same functions in the same order, flies the same bundles on
the same waves in the same rounds, and differs from the general kernel in what
it knows at compile time. So against `bundle_march=0` the total weight, the
four type counts, the DDA step count and the wave-step count are EXACTLY equal
and J_H differs by the order of the atomic adds only: rtol 1e-11 per cell, the
tolerance of test_gpu_span_schedule.py for "same packets, other order of
atomic adds".

class_group_chunks changes the order of the packets only: counts and steps
exactly equal, J_H at the same tolerance; how many trips the waves make does
change, and is printed."""
import numpy as np
import pytest

from test_gpu_transport import make_engine
from test_gpu_march_records import noncubic_engine

pytestmark = pytest.mark.gpu

# one wave's chunk is 64 positions, a block's span 8 chunks = 512: the
# smallest launch, the chunk's and the span's edges, fewer chunks than a block
# has waves with a short last span, many spans
COUNTS = [1, 63, 64, 65, 511, 512, 513, 4097, 100003]
# 586 spans, the last short, for at most one block per CU: span after span
# across the XCDs' cursors
MANY_SPANS = 300003
FIRST_PAD = 2

BASE = dict(bundle_march=1, pad_march=1, pad_uniform=1, span_claim=1,
            emit_before_flush=1, xcd_remap=0, chunk=64, refill_threshold=64,
            max_packets_per_launch=1 << 27, max_blocks_per_cu=8,
            class_group_chunks=1, sort_tau_bits=-1, sort_dir_bits=-1)

_engines = {}
_reference = {}


def engine(kind):
    """One engine per set-up, shared by the module's tests."""
    from cmacionize_amd import STROMGREN as S
    from cmacionize_amd import engine as E
    if kind in _engines:
        return _engines[kind]
    side = S["sides"][0]
    if kind == "plain16":
        eng = make_engine(16, track_heating=False)
    elif kind == "plain24":
        eng = make_engine(24, track_heating=False)
    elif kind == "heating16":
        eng = make_engine(16, track_heating=True)
    elif kind == "noncubic":
        # 24 x 16 x 20 cells, a slab of vacuum, a star off the centre
        eng = noncubic_engine(False)
    elif kind == "outside16":
        # a star outside the box: every flight ends at once
        eng = make_engine(16, track_heating=False)
        eng.set_sources([[0.9 * side, 0.1 * side, -0.2 * side]], [1.],
                        S["luminosity"])
    elif kind == "twostars16":
        eng = make_engine(16, track_heating=False)
        eng.set_sources([[0.21 * side, -0.13 * side, 0.07 * side],
                         [-0.17 * side, 0.09 * side, -0.23 * side]],
                        [0.5, 0.5], S["luminosity"])
    elif kind == "mixed16":
        # a star and a continuous source of 2.5 times its luminosity: two
        # photon weights, the build with a product per lane
        eng = make_engine(16, track_heating=False)
        eng.set_continuous_spectrum_monochromatic(1.1 * S["frequency"])
        eng.set_continuous_source(E.CONTINUOUS_ISOTROPIC,
                                  2.5 * S["luminosity"])
    elif kind == "equal16":
        # ... of the star's luminosity: one weight, the UNIFORM build
        eng = make_engine(16, track_heating=False)
        eng.set_continuous_spectrum_monochromatic(1.1 * S["frequency"])
        eng.set_continuous_source(E.CONTINUOUS_ISOTROPIC, S["luminosity"])
    elif kind == "reemission16":
        eng = make_engine(16, track_heating=False)
        eng.set_reemission(1)
    elif kind == "block24":
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
    settings = dict(BASE)
    settings.update(tuning)
    eng.set_tuning(**settings)
    eng.reset_grid()
    if kind == "block24":
        eng.reset_exports()
    eng.shoot(11, 2, 5, n)
    tw, tc, ns = eng.get_counters()
    out = dict(tw=tw, tc=tc, ns=ns, ws=eng.get_wave_steps(),
               plan=eng.transport_plan(), bundle=eng.bundle_march_flown(),
               atomics=eng.get_atomic_count(),
               J=eng.download_field(E.FIELD_MEAN_INTENSITY))
    if kind == "block24":
        out["exports"] = eng.get_export_count()
    return out


def general(kind, n, **tuning):
    """The general kernel with the same settings, once per case; left
    unchanged."""
    key = (kind, n) + tuple(sorted(tuning.items()))
    if key not in _reference:
        ref = shoot(kind, n, **dict(tuning, bundle_march=0))
        assert not ref["bundle"]
        _reference[key] = ref
    return _reference[key]


def check_same(got, ref, n=None, wave_steps=True):
    print("tw", got["tw"], ref["tw"], "tc", got["tc"], ref["tc"], "ns",
          got["ns"], ref["ns"], "ws", got["ws"], ref["ws"])
    if n is not None:
        assert ref["tw"] == n
    assert got["tw"] == ref["tw"]
    assert np.array_equal(got["tc"], ref["tc"])
    assert got["ns"] == ref["ns"]
    if wave_steps:
        assert got["ws"] == ref["ws"]
    a, b = got["J"], ref["J"]
    nz = b != 0.
    print("J_H max relative difference",
          np.abs(a[nz] / b[nz] - 1.).max() if nz.any() else 0.)
    assert np.allclose(a, b, rtol=1e-11, atol=1e-13 * np.abs(b).max())
    assert ref["J"].max() > 0. or ref["ns"] == 0
    if "exports" in ref:
        assert got["exports"] == ref["exports"]


def check_bundle(kind, n, uniform=True, total=True, **tuning):
    got = shoot(kind, n, **tuning)
    assert got["bundle"]
    assert got["plan"] == (FIRST_PAD, uniform)
    ref = general(kind, n, **tuning)
    assert ref["plan"] == (FIRST_PAD, uniform)
    check_same(got, ref, n if total else None)
    return got


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("xcd_remap", [0, 1])
@pytest.mark.parametrize("kind", ["plain16", "plain24"])
def test_bundle_build_equals_the_general_kernel(kind, xcd_remap, n):
    check_bundle(kind, n, xcd_remap=xcd_remap)


@pytest.mark.parametrize("emit_before_flush", [0, 1])
@pytest.mark.parametrize("xcd_remap", [0, 1])
def test_span_after_span_at_one_block_per_cu(xcd_remap, emit_before_flush):
    check_bundle("plain24", MANY_SPANS, xcd_remap=xcd_remap,
                 emit_before_flush=emit_before_flush, max_blocks_per_cu=1)


@pytest.mark.parametrize("n", COUNTS)
def test_several_launches_in_one_call(n):
    """(1024 is the least a launch can be limited to)"""
    check_bundle("plain24", n, xcd_remap=1, max_packets_per_launch=1024)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", ["plain16", "plain24"])
def test_flush_point_ahead_of_the_refill(kind, n):
    check_bundle(kind, n, emit_before_flush=0)


@pytest.mark.parametrize("n", [1, 65, 513, 4097, 100003])
@pytest.mark.parametrize("kind,uniform", [("noncubic", True),
                                          ("outside16", True),
                                          ("twostars16", True),
                                          ("mixed16", False),
                                          ("equal16", True)])
def test_other_grids_and_sources(kind, uniform, n):
    got = check_bundle(kind, n, uniform=uniform, total=kind != "mixed16")
    if kind == "outside16":
        assert got["ns"] == 0 and not got["J"].any()
        assert got["tc"][0] == n          # all left as they came
    if kind == "noncubic" and n >= 4097:
        J = got["J"].reshape(24, 16, 20)
        assert not J[17:19].any() and J[19:].any()
    if kind == "mixed16" and n >= 4097:
        # packets of both sources, and both weights in the total
        assert n < got["tw"] < 2.5 * n


@pytest.mark.parametrize("n", COUNTS)
def test_product_per_lane_where_the_uniform_build_is_off(n):
    check_bundle("plain16", n, uniform=False, pad_uniform=0)


@pytest.mark.parametrize("n", [513, 20000])
def test_bundle_build_matches_oracle(oracle, n):
    sim = oracle.stromgren_simulation(16)
    sim.reset()
    sim.totweight = 0.
    sim.typecount[:] = 0.
    sim.shoot(11, 2, 5, n)
    got = shoot("plain16", n)
    assert got["bundle"]
    assert got["tw"] == sim.totweight == n
    assert np.array_equal(got["tc"], sim.typecount)
    assert np.allclose(got["J"], sim.J[0], rtol=1e-9,
                       atol=1e-12 * sim.J[0].max())


def test_bundle_build_is_the_default():
    """An engine nobody has tuned."""
    fresh = make_engine(16, track_heating=False)
    try:
        fresh.reset_grid()
        fresh.shoot(11, 2, 5, 4097)
        assert fresh.bundle_march_flown()
        assert fresh.transport_plan() == (FIRST_PAD, True)
    finally:
        fresh.close()


@pytest.mark.parametrize("kind,tuning", [
    ("plain16", dict(chunk=128)),
    ("plain16", dict(refill_threshold=32)),
    ("plain16", dict(span_claim=0)),
    ("heating16", dict()),
    ("reemission16", dict()),
    ("block24", dict()),
])
def test_everything_else_keeps_the_general_kernel(kind, tuning):
    """... and flies what it flew with bundle_march=0."""
    for n in (65, 4097, 100003):
        got = shoot(kind, n, **tuning)
        assert not got["bundle"]
        ref = general(kind, n, **tuning)
        assert got["plan"] == ref["plan"]
        # (later generations refill from a queue that atomics fill: how many
        # trips their waves make differs from one run to the next of the
        # same kernel - seen: 25511 and 25518)
        check_same(got, ref, wave_steps=kind != "reemission16")


# ---- class_group_chunks ----------------------------------------------------

@pytest.mark.parametrize("n", [100000, (1 << 20) + 37])
def test_class_groups_of_eight_chunks(n):
    """3 class bits; the larger count takes the bucket order (1e6 packets and
    more, with a 16-bit key: 13 direction bits, as test_gpu_packet_order.py
    has it)."""
    from cmacionize_amd import engine as E
    eng = engine("plain24")
    results = {}
    keys_of = dict(sort_tau_bits=3)
    if n >= 1000000:
        keys_of["sort_dir_bits"] = 13
    for g in (1, 8):
        eng.set_tuning(**dict(BASE, class_group_chunks=g, **keys_of))
        ids, keys = eng.order_packets(11, 2, 5, n)
        path, _, _, overflow = eng.order_plan()
        assert path == (E.ORDER_BUCKET if n >= 1000000 else E.ORDER_RADIX)
        assert overflow == 0
        assert np.array_equal(np.sort(ids), np.arange(n, dtype=np.uint32))
        pair = (keys.astype(np.uint64) << np.uint64(32)) | ids
        assert np.all(pair[1:] > pair[:-1])
        results[g] = shoot("plain24", n, class_group_chunks=g, **keys_of)
        assert results[g]["bundle"]
    print("wave steps with class_group_chunks 1 / 8:", results[1]["ws"],
          results[8]["ws"], "atomics:", results[1]["atomics"],
          results[8]["atomics"])
    check_same(results[8], results[1], n, wave_steps=False)
