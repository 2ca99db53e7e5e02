"""GPU tests of the bucket order (tuning key bucket_order, packet_order.h): the
packets of a hydrogen-only launch by sort key through two scatter levels and
a sort of the leaves in LDS, against key kernel and radix sort.

The probe (GpuEngine.order_packets) runs the ordering stage of a launch by
the plan of a shoot and returns the order with the keys of the ordered
packets. Without overflow the two orders are the same word for word: both
sort by (key, id). With a region or a leaf too small for its share the order
is still a permutation of the launch's ids - those that found no room follow
the ordered ones - and the plan query reports how many.

Small launches reach full-size leaves through the tuning keys: 13 direction
bits and 3 class bits (16 key bits), 5 + 5 bits for the two levels, so that
2^20 packets are 1024 leaves of 1024 pairs."""
import numpy as np
import pytest

from test_gpu_transport import make_engine

pytestmark = pytest.mark.gpu

# one packet; below, at and above a wave; below and above a tile of 4096 (the
# last tile short, most regions and leaves empty); full-size leaves
COUNTS = [1, 63, 64, 65, 4095, 4097, (1 << 20) + 37]
FULL = COUNTS[-1]
KEYS = dict(sort_dir_bits=13, sort_tau_bits=3, bucket_bits1=5, bucket_bits2=5,
            bucket_min_packets=0, bucket_slack_permille=-1,
            max_packets_per_launch=1 << 27)
SEED, ITERATION, FIRST = 11, 2, 5

_engines = {}
_radix = {}


def engine(kind):
    """One engine per set-up, shared by the module's tests."""
    if kind in _engines:
        return _engines[kind]
    from cmacionize_amd import STROMGREN as S
    if kind == "one":
        eng = make_engine(16, track_heating=False)
    elif kind == "two":
        # two sources: a source bit on top of the key, and 99 in 100 packets
        # in the regions of the first
        eng = make_engine(16, track_heating=False)
        side = S["sides"][0]
        eng.set_sources([[0., 0., 0.], [0.2 * side, 0.1 * side, 0.]],
                        [0.99, 0.01], S["luminosity"])
    elif kind == "grid32":
        eng = make_engine(32, track_heating=False)
    else:
        raise KeyError(kind)
    _engines[kind] = eng
    return eng


@pytest.fixture(scope="module", autouse=True)
def close_engines():
    yield
    for eng in _engines.values():
        eng.close()
    _engines.clear()
    _radix.clear()


def order(kind, n, bucket, **tuning):
    """(ids, keys, plan) of the launch's order by either path."""
    from cmacionize_amd import engine as E
    eng = engine(kind)
    settings = dict(KEYS)
    settings.update(tuning)
    eng.set_tuning(bucket_order=bucket, **settings)
    ids, keys = eng.order_packets(SEED, ITERATION, FIRST, n)
    plan = eng.order_plan()
    assert plan[0] == (E.ORDER_BUCKET if bucket else E.ORDER_RADIX)
    return ids, keys, plan


def radix(kind, n):
    """The radix sort's order, once per set-up and count."""
    if (kind, n) not in _radix:
        ids, keys, plan = order(kind, n, 0)
        assert plan[1:] == (0, 0, 0)
        # the reference itself: every id once, by (key, id)
        assert np.array_equal(np.sort(ids), np.arange(n, dtype=np.uint32))
        pair = (keys.astype(np.uint64) << np.uint64(32)) | ids
        assert np.all(pair[1:] > pair[:-1])
        _radix[(kind, n)] = (ids, keys)
    return _radix[(kind, n)]


def check_overflowed(ids, keys, plan, n):
    """A permutation; ordered by (key, id) ahead of a tail of plan[3] ids."""
    overflow = plan[3]
    print("n %d: %d + %d bits, %d of the packets overflowed"
          % (n, plan[1], plan[2], overflow))
    assert np.array_equal(np.sort(ids), np.arange(n, dtype=np.uint32))
    assert 0 < overflow <= n
    head = n - overflow
    pair = (keys[:head].astype(np.uint64) << np.uint64(32)) | ids[:head]
    assert np.all(pair[1:] > pair[:-1])
    # (the callers: the head is the radix sort's order with exactly the ids
    # of the tail taken out)
    return head


@pytest.mark.parametrize("n", COUNTS)
def test_bucket_order_equals_the_radix_sort(n):
    ref_ids, ref_keys = radix("one", n)
    ids, keys, plan = order("one", n, 1)
    assert plan[1:] == (5, 5, 0)
    # no id is missing (empty leaves, a last tile shorter than a tile) ...
    assert np.array_equal(np.sort(ids), np.arange(n, dtype=np.uint32))
    # ... and every one is where the stable radix sort puts it
    assert np.array_equal(ids, ref_ids)
    assert np.array_equal(keys, ref_keys)


def test_bucket_order_by_its_own_choice_of_bits():
    """No bits forced: 2^20 packets with 16-bit keys are 10 bits, 5 + 5."""
    ref_ids, _ = radix("one", FULL)
    ids, _, plan = order("one", FULL, 1, bucket_bits1=-1, bucket_bits2=-1)
    assert plan[1:] == (5, 5, 0)
    assert np.array_equal(ids, ref_ids)


@pytest.mark.parametrize("n", [4097, FULL])
def test_overflow_of_regions_and_leaves_is_an_order(n):
    """No room beyond the mean: about half the regions and leaves overflow."""
    ids, keys, plan = order("one", n, 1, bucket_slack_permille=0)
    head = check_overflowed(ids, keys, plan, n)
    # what is ordered is ordered as the radix sort orders it: the head is the
    # radix order with the overflowed ids taken out
    ref_ids, _ = radix("one", n)
    kept = np.ones(n, dtype=bool)
    kept[ids[head:]] = False
    assert np.array_equal(ids[:head], ref_ids[kept[ref_ids]])


def test_overflow_of_skewed_regions_is_an_order():
    """Two sources of weights 0.99 and 0.01 with the default room: the
    regions of the first source hold half of what they are sent."""
    n = FULL
    ref_ids, ref_keys = radix("two", n)
    assert ref_keys.max() >> 16 == 1  # the source bit
    ids, keys, plan = order("two", n, 1)
    head = check_overflowed(ids, keys, plan, n)
    assert plan[3] > n // 4
    kept = np.ones(n, dtype=bool)
    kept[ids[head:]] = False
    assert np.array_equal(ids[:head], ref_ids[kept[ref_ids]])


def test_one_transport_call_by_either_order():
    """32^3 cells, 2e5 packets: the same flights in the same bundles."""
    from cmacionize_amd import engine as E
    eng = engine("grid32")
    n = 200000
    got = {}
    for bucket in (0, 1):
        eng.set_tuning(bucket_order=bucket, **dict(KEYS, bucket_bits1=4,
                                                   bucket_bits2=4))
        eng.reset_grid()
        eng.shoot(SEED, ITERATION, FIRST, n)
        tw, tc, ns = eng.get_counters()
        plan = eng.order_plan()
        assert plan[0] == (E.ORDER_BUCKET if bucket else E.ORDER_RADIX)
        assert plan[3] == 0
        got[bucket] = dict(tw=tw, tc=tc, ns=ns, waves=eng.get_wave_steps(),
                           J=eng.download_field(E.FIELD_MEAN_INTENSITY))
    ref, new = got[0], got[1]
    assert ref["tw"] == new["tw"] == n
    assert np.array_equal(ref["tc"], new["tc"])
    assert ref["ns"] == new["ns"] > 0
    assert ref["waves"] == new["waves"]
    # (the sums differ by the order of the atomic adds only: the tolerance of
    # test_gpu_bundle_order.py)
    assert ref["J"].max() > 0.
    assert np.allclose(new["J"], ref["J"], rtol=1e-11,
                       atol=1e-13 * ref["J"].max())


def test_plan_query_reports_the_path():
    from cmacionize_amd import engine as E
    from cmacionize_amd import GpuEngine, STROMGREN as S
    from cmacionize_amd.simulation import DomainDecomposition, DomainGpuBackend
    from test_gpu_domain import configure, lexington_fields
    forced = dict(KEYS, bucket_order=1)
    n = 20000
    # hydrogen only, an undivided grid: the bucket order, also in a shoot
    eng = engine("one")
    eng.set_tuning(**forced)
    eng.reset_grid()
    eng.shoot(SEED, ITERATION, FIRST, n)
    assert eng.order_plan() == (E.ORDER_BUCKET, 5, 5, 0)
    # ... below the size threshold the radix sort, unsorted no order at all
    eng.set_tuning(bucket_min_packets=n + 1)
    eng.shoot(SEED, ITERATION, FIRST, n)
    assert eng.order_plan() == (E.ORDER_RADIX, 0, 0, 0)
    eng.set_tuning(sort_packets=0)
    eng.shoot(SEED, ITERATION, FIRST, n)
    assert eng.order_plan() == (E.ORDER_NONE, 0, 0, 0)
    eng.set_tuning(sort_packets=1)
    # multi-ion: the classes are octaves of a range, not uniform
    dens, temp = lexington_fields(8)
    lex = GpuEngine((8,) * 3, S["anchor"], S["sides"], (0, 0, 0), device=0,
                    track_heating=True)
    try:
        configure(lex, "lexington", 8 ** 3, dens.ravel(), temp.ravel())
        lex.set_tuning(**dict(forced, sort_tau_bits=2))
        lex.reset_grid()
        lex.shoot(SEED, ITERATION, FIRST, n)
        assert lex.order_plan() == (E.ORDER_RADIX, 0, 0, 0)
    finally:
        lex.close()
    # a block of a decomposed grid orders its selection of the launch's ids
    dec = DomainDecomposition((24,) * 3, (3, 1, 1))
    backend = DomainGpuBackend(dec, 1, S["anchor"], S["sides"], device=0,
                               track_heating=False, export_capacity=1 << 19)
    block = backend.engine
    try:
        configure(block, "stromgren", int(np.prod(dec.block(1)[1])))
        block.set_tuning(**forced)
        block.reset_grid()
        block.reset_exports()
        block.shoot(SEED, ITERATION, FIRST, n)
        assert block.order_plan() == (E.ORDER_RADIX, 0, 0, 0)
    finally:
        block.close()
