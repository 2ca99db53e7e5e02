"""With one discrete source and no continuous source the first two uniforms of
a packet - "continuous or discrete?", "which source?" - decide nothing, and
their Philox block is passed over instead of generated. The same model with
its source given twice at the same position, with weights (1, 0), has two
sources: it draws both uniforms and always picks source 0. Every later draw of
a packet must be what it was - packets, counters and mean intensities of the
two forms are equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def make_engine(ncell, twice):
    from cmacionize_amd import GpuEngine, STROMGREN as S
    eng = GpuEngine((ncell,) * 3, S["anchor"], S["sides"], S["periodic"],
                    device=0, track_heating=False)
    position = [0.11 * S["sides"][0], -0.07 * S["sides"][0],
                0.03 * S["sides"][0]]
    if twice:
        eng.set_sources([position, position], [1., 0.], S["luminosity"])
    else:
        eng.set_sources([position], [1.], S["luminosity"])
    eng.set_spectrum_monochromatic(S["frequency"])
    sigma = np.zeros(14)
    sigma[0] = S["sigma_H"]
    alpha = np.zeros(14)
    alpha[0] = S["alpha_H"]
    eng.set_cross_sections_fixed(sigma)
    eng.set_recombination_rates_fixed(alpha)
    n = ncell ** 3
    x = np.zeros((14, n))
    x[0] = 2.e-5  # thin enough that packets cross many cells
    x[1] = S["xHe"]
    eng.upload_cells(np.full(n, S["density"]), np.full(n, S["temperature"]), x)
    return eng


def test_emitted_packets_are_the_same():
    one, two = make_engine(8, False), make_engine(8, True)
    a = one.emit_packets(42, 3, 0, 4096)
    b = two.emit_packets(42, 3, 0, 4096)
    one.close()
    two.close()
    for got, want in zip(a, b):
        assert np.array_equal(got, want)
    assert np.unique(a[1][:, 0]).size > 4000  # directions were drawn


def shoot_once(twice, tuning, reemission):
    from cmacionize_amd import engine as E
    eng = make_engine(16, twice)
    if reemission:
        eng.set_reemission(1)
    eng.set_tuning(**tuning)
    eng.reset_grid()
    eng.shoot(42, 1, 0, 200000)
    counters = eng.get_counters()
    J = eng.download_field(E.FIELD_MEAN_INTENSITY)
    eng.close()
    return counters, J


@pytest.mark.parametrize("reemission", [False, True])
@pytest.mark.parametrize("sort_packets", [1, 0])
def test_one_iteration_is_the_same(sort_packets, reemission):
    """The key kernel (sorted runs) and the transport kernel pass over the
    block; with re-emission the streams are resumed later from the block
    count the first generation left."""
    tuning = dict(sort_packets=sort_packets)
    (tw1, tc1, ns1), J1 = shoot_once(False, tuning, reemission)
    (tw2, tc2, ns2), J2 = shoot_once(True, tuning, reemission)
    assert tw1 == tw2 == 200000
    assert np.array_equal(tc1, tc2), (tc1, tc2)
    assert ns1 == ns2
    if reemission:
        assert tc1[1] > 0  # some packets were re-emitted
    # (the order of the atomic additions is not reproducible)
    assert J1.max() > 0.
    assert np.allclose(J1, J2, rtol=1e-12, atol=0.)
