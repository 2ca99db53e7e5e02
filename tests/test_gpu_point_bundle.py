"""GPU tests of the point build of the bundle kernel (tuning key bundle_point;
shoot_bundle_kernel<true, true>).

The point build flies launches whose packets all come from ONE discrete source
with no continuous one. It emits every packet from the same draws with the
same operations on the same operands as the bundle build and the general
kernel - the walls of the source's cell relative to the source are computed
once per launch instead of per packet, by start_flight itself - and flies the
same bundles on the same waves in the same rounds. So against `bundle_point=0`
and against `bundle_march=0` the total weight, the four type counts, the DDA
step count and the wave-step count are EXACTLY equal, and J_H differs by the
order of the atomic adds only: rtol 1e-11 per cell, the project's tolerance
for "same packets, other order of atomic adds" (test_gpu_bundle_march.py,
whose helpers these tests build on)."""
import numpy as np
import pytest

import test_gpu_bundle_march as b
from test_gpu_transport import make_engine

pytestmark = pytest.mark.gpu

COUNTS = b.COUNTS
FIRST_PAD = b.FIRST_PAD
PC = 3.086e16

_other = {}


def engine(kind):
    """The set-ups of test_gpu_bundle_march.py and three more stars."""
    from cmacionize_amd import STROMGREN as S
    if kind in b._engines:
        return b._engines[kind]
    if kind == "corner16":
        # in the last cell of the grid along every axis: the largest padded
        # offset, ghost cells one step away
        eng = make_engine(16, track_heating=False)
        eng.set_sources([[4.9 * PC, 4.8 * PC, 4.7 * PC]], [1.],
                        S["luminosity"])
    elif kind == "face16":
        # exactly on the low x face of the box (inside: cell 0 along x), off
        # the walls along y and z
        eng = make_engine(16, track_heating=False)
        eng.set_sources([[-5. * PC, 1.3 * PC, -2.1 * PC]], [1.],
                        S["luminosity"])
    elif kind == "planck16":
        # a Planck star: one more draw per packet, the optical depth's is the
        # second of its Philox block
        eng = make_engine(16, track_heating=False)
        eng.set_spectrum_planck(40000.)
    else:
        return b.engine(kind)
    b._engines[kind] = eng
    return eng


@pytest.fixture(scope="module", autouse=True)
def close_engines():
    yield
    for key, eng in b._engines.items():
        if not key.endswith(":backend"):
            eng.close()
    b._engines.clear()
    b._reference.clear()
    _other.clear()


def shoot(kind, n, **tuning):
    eng = engine(kind)
    out = b.shoot(kind, n, **tuning)
    out["point"] = eng.bundle_point_flown()
    return out


def others(kind, n, **tuning):
    """The bundle build and the general kernel with the same settings, once
    per case; left unchanged."""
    key = (kind, n) + tuple(sorted(tuning.items()))
    if key not in _other:
        bundle = shoot(kind, n, **dict(tuning, bundle_point=0))
        assert bundle["bundle"] and not bundle["point"]
        general = shoot(kind, n, **dict(tuning, bundle_point=1,
                                        bundle_march=0))
        assert not general["bundle"] and not general["point"]
        _other[key] = (bundle, general)
    return _other[key]


def check_point(kind, n, total=True, **tuning):
    got = shoot(kind, n, **dict(tuning, bundle_point=1))
    assert got["point"] and got["bundle"]
    assert got["plan"] == (FIRST_PAD, True)
    for ref in others(kind, n, **tuning):
        assert ref["plan"] == (FIRST_PAD, True)
        b.check_same(got, ref, n if total else None)
    return got


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", ["plain16", "plain24", "noncubic",
                                  "outside16", "corner16", "face16",
                                  "planck16"])
def test_point_build_equals_the_bundle_build_and_the_general_kernel(kind, n):
    got = check_point(kind, n)
    if kind == "outside16":
        assert got["ns"] == 0 and not got["J"].any()
        assert got["tc"][0] == n          # all left as they came
    else:
        assert got["ns"] > 0 and got["J"].any()
    if kind == "noncubic" and n >= 4097:
        J = got["J"].reshape(24, 16, 20)
        assert not J[17:19].any() and J[19:].any()


@pytest.mark.parametrize("n", [4097, 100003])
def test_several_launches_in_one_call(n):
    """(1024 is the least a launch can be limited to: a block per launch)"""
    check_point("plain24", n, max_packets_per_launch=1024)


@pytest.mark.parametrize("emit_before_flush", [0, 1])
@pytest.mark.parametrize("n", [513, 100003])
def test_with_the_blocks_dealt_by_xcd(n, emit_before_flush):
    check_point("plain24", n, xcd_remap=1,
                emit_before_flush=emit_before_flush)


def result(eng, n, **tuning):
    from cmacionize_amd import engine as E
    eng.set_tuning(**dict(b.BASE, **tuning))
    eng.reset_grid()
    eng.shoot(11, 2, 5, n)
    tw, tc, ns = eng.get_counters()
    return dict(tw=tw, tc=tc, ns=ns, ws=eng.get_wave_steps(),
                plan=eng.transport_plan(), bundle=eng.bundle_march_flown(),
                point=eng.bundle_point_flown(),
                J=eng.download_field(E.FIELD_MEAN_INTENSITY))


def test_sources_set_again_between_two_calls():
    """The block holds the source's cell and walls: a second call after
    cmi_gpu_set_sources must start from the new star."""
    from cmacionize_amd import STROMGREN as S
    n = 100003
    eng = make_engine(16, track_heating=False)
    try:
        first = result(eng, n, bundle_point=1)
        assert first["point"]
        eng.set_sources([[1.7 * PC, -3.3 * PC, 4.1 * PC]], [1.],
                        S["luminosity"])
        second = result(eng, n, bundle_point=1)
        assert second["point"]
        bundle = result(eng, n, bundle_point=0)
        assert bundle["bundle"] and not bundle["point"]
        general = result(eng, n, bundle_march=0)
        assert not general["bundle"]
        b.check_same(second, bundle, n)
        b.check_same(second, general, n)
        assert second["ns"] != first["ns"]
    finally:
        eng.close()


def test_cell_update_between_two_calls():
    """The block holds the record of the star's cell: a second call after an
    update of the cells must read the record the update left."""
    from cmacionize_amd import engine as E
    n = 100003
    eng = make_engine(16, track_heating=False)
    try:
        first = result(eng, n, bundle_point=1)
        assert first["point"]
        eng.upload_field(E.FIELD_MEAN_INTENSITY, first["J"])
        eng.update_cells(0, float(n))
        second = result(eng, n, bundle_point=1)
        assert second["point"]
        bundle = result(eng, n, bundle_point=0)
        assert bundle["bundle"] and not bundle["point"]
        general = result(eng, n, bundle_march=0)
        assert not general["bundle"]
        b.check_same(second, bundle, n)
        b.check_same(second, general, n)
        # (other neutral fractions: the flights end elsewhere)
        assert second["ns"] != first["ns"]
    finally:
        eng.close()


@pytest.mark.parametrize("kind,bundle", [("twostars16", True),
                                         ("mixed16", True),
                                         ("equal16", True),
                                         ("reemission16", False),
                                         ("heating16", False),
                                         ("block24", False)])
def test_everything_else_keeps_the_kernel_it_had(kind, bundle):
    """Two stars, a continuous source (of another weight and of the star's),
    re-emission, the heating term, a block of a decomposed grid: the plan
    says that the point build was not taken, and the launch flies what it
    flew with bundle_point=0."""
    for n in (65, 4097, 100003):
        got = shoot(kind, n, bundle_point=1)
        assert not got["point"]
        assert got["bundle"] == bundle
        ref = shoot(kind, n, bundle_point=0)
        assert not ref["point"]
        assert got["plan"] == ref["plan"]
        # (later generations refill from a queue that atomics fill: how many
        # trips their waves make differs from one run to the next)
        b.check_same(got, ref, wave_steps=kind != "reemission16")


def test_switched_off_it_is_the_bundle_build():
    got = shoot("plain16", 4097, bundle_point=0)
    assert got["bundle"] and not got["point"]
    got = shoot("plain16", 4097, bundle_point=1, bundle_march=0)
    assert not got["bundle"] and not got["point"]


def test_point_build_is_the_default():
    """An engine nobody has tuned."""
    fresh = make_engine(16, track_heating=False)
    try:
        fresh.reset_grid()
        fresh.shoot(11, 2, 5, 4097)
        assert fresh.bundle_point_flown() and fresh.bundle_march_flown()
        assert fresh.transport_plan() == (FIRST_PAD, True)
    finally:
        fresh.close()


@pytest.mark.parametrize("n", [513, 20000])
def test_point_build_matches_oracle(oracle, n):
    sim = oracle.stromgren_simulation(16)
    sim.reset()
    sim.totweight = 0.
    sim.typecount[:] = 0.
    sim.shoot(11, 2, 5, n)
    got = shoot("plain16", n, bundle_point=1)
    assert got["point"]
    assert got["tw"] == sim.totweight == n
    assert np.array_equal(got["tc"], sim.typecount)
    assert np.allclose(got["J"], sim.J[0], rtol=1e-9,
                       atol=1e-12 * sim.J[0].max())
