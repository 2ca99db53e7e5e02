"""GPU tests of the escape maps: the tally of the transport kernels against
the plain-C restatement bin for bin, against the numpy form of the header's
formula, against ray tracing, its switches, the blocks of a decomposed grid
and the .param driver."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import escape_lib as X  # noqa: E402

pytestmark = pytest.mark.gpu


def set_tally(eng, bins, frame, nlon=X.NLON, nmu=X.NMU):
    kind, nfreq, fmin, fmax = bins
    if kind == "Level":
        eng.set_escape_tally(nlon, nmu, frame, bins="Level")
    else:
        eng.set_escape_tally(nlon, nmu, frame, nfreq=nfreq,
                             minimum_frequency=fmin, maximum_frequency=fmax)


# 1. parity, bin for bin ------------------------------------------------------
@pytest.mark.parametrize("bins", [X.LINEAR_BINS, X.LEVEL_BINS],
                         ids=["linear", "level"])
@pytest.mark.parametrize("passes", [1, 0])
def test_tally_equals_restatement_on_lexington(oracle, passes, bins):
    """The 20^3 lexington state, re-emission on, temperature solve off, 40000
    packets, 12 x 6 pixels in a tilted frame: the engine's array equals the
    restatement's, bin for bin, no packet excused - which the restatement's
    edge distances make safe."""
    frame = X.tilted_frame()
    sky, tw, tc, edge = X.lexington_reference(bins)
    assert edge[0] > X.EDGE_MARGIN and edge[1] > X.EDGE_MARGIN, edge
    eng = X.lexington_engine(X.lexington_state(), reemit_passes=passes)
    set_tally(eng, bins, frame)
    eng.enable_trackers(True)
    eng.reset_grid()
    eng.shoot(X.LEX_SEED, 1, 0, X.LEX_PACKETS)
    gtw, gtc, _ = eng.get_counters()
    got = eng.escape_tally()
    eng.close()
    assert got.shape == sky.shape == (3, bins[1], X.NLON, X.NMU)
    assert gtw == tw == X.LEX_PACKETS
    assert np.array_equal(gtc, tc)
    assert np.array_equal(got.sum(axis=(1, 2, 3)), gtc[:3])
    assert np.array_equal(got, sky), np.argwhere(got != sky)[:10]
    assert gtc[0] > 0 and gtc[1] > 0 and gtc[2] > 0


@pytest.mark.parametrize("passes", [1, 0])
def test_tally_equals_restatement_on_the_periodic_box(oracle, passes):
    """The periodic Stromgren case (16^3, x and y periodic, hydrogen only,
    diffuse re-emission): a periodic face is never left."""
    sim, source = X.periodic_simulation()
    sky, tw, tc, edge = X.shoot(sim, X.PERIODIC_SEED, 0, 0,
                                X.PERIODIC_PACKETS, X.NLON, X.NMU,
                                X.tilted_frame(), X.LINEAR_BINS)
    assert edge[0] > X.EDGE_MARGIN and edge[1] > X.EDGE_MARGIN, edge
    fresh, _ = X.periodic_simulation()
    eng = X.periodic_engine(fresh, source, reemit_passes=passes)
    set_tally(eng, X.LINEAR_BINS, X.tilted_frame())
    eng.enable_trackers(True)
    eng.reset_grid()
    eng.shoot(X.PERIODIC_SEED, 0, 0, X.PERIODIC_PACKETS)
    gtw, gtc, _ = eng.get_counters()
    got = eng.escape_tally()
    eng.close()
    assert gtw == tw == X.PERIODIC_PACKETS
    assert np.array_equal(gtc, tc)
    assert np.array_equal(got.sum(axis=(1, 2, 3)), gtc[:3])
    assert np.array_equal(got, sky), np.argwhere(got != sky)[:10]
    assert gtc[0] > 0 and gtc[1] > 0


# 2. the mapping, independent of the restatement ------------------------------
def vacuum_engine(ncell=8):
    from cmacionize_amd import GpuEngine, STROMGREN as S
    eng = GpuEngine((ncell,) * 3, S["anchor"], S["sides"], (0, 0, 0),
                    device=0)
    eng.set_sources([[0.11 * S["sides"][0], -0.23 * S["sides"][0],
                      0.07 * S["sides"][0]]], [1.], S["luminosity"])
    eng.set_spectrum_monochromatic(S["frequency"])
    sigma = np.zeros(14)
    sigma[0] = S["sigma_H"]
    alpha = np.zeros(14)
    alpha[0] = S["alpha_H"]
    eng.set_cross_sections_fixed(sigma)
    eng.set_recombination_rates_fixed(alpha)
    n = ncell ** 3
    x = np.zeros((14, n))
    x[0] = 1.e-6
    eng.upload_cells(np.zeros(n), np.zeros(n), x)
    return eng


def test_vacuum_box_maps_every_direction_to_its_pixel():
    """A box of vacuum: every packet leaves with the direction it was emitted
    with. The tally is the numpy binning of emit_packets' directions by the
    header's formula, and it is uniform over the equal-area pixels."""
    npacket, seed = 72000, 17
    frame = X.tilted_frame()
    eng = vacuum_engine()
    eng.set_escape_tally(X.NLON, X.NMU, frame)
    eng.enable_trackers(True)
    eng.reset_grid()
    eng.shoot(seed, 0, 0, npacket)
    tw, tc, _ = eng.get_counters()
    got = eng.escape_tally()
    _, d, _, _, _ = eng.emit_packets(seed, 0, 0, npacket)
    eng.close()
    assert got.shape == (3, 1, X.NLON, X.NMU)
    assert tw == npacket and tc[0] == npacket
    assert got.sum() == npacket and got[1:].sum() == 0
    pix, dist = X.numpy_pixels(d, X.NLON, X.NMU, frame)
    # directions within 1e-9 of an edge would be left out: there are none
    assert (dist > X.EDGE_MARGIN).all(), np.sort(dist)[:5]
    want = np.bincount(pix, minlength=X.NLON * X.NMU).reshape(X.NLON, X.NMU)
    assert np.array_equal(got[0, 0], want)
    # chi-square against uniform: 72 pixels, 71 degrees of freedom
    expected = npacket / (X.NLON * X.NMU)
    chi2 = ((got[0, 0] - expected) ** 2 / expected).sum()
    print("chi-square %.2f, bound %.2f" % (chi2,
                                           X.chi2_quantile(1. - 1e-6, 71)))
    assert chi2 < X.chi2_quantile(1. - 1e-6, 71)


# 3. against ray tracing ------------------------------------------------------
def sub_rays(nlon, nmu, S, frame):
    """S x S sub-rays per pixel, uniform in (l, mu): (nlon * nmu, S * S, 3)"""
    f = np.asarray(frame, dtype=np.float64)
    i = np.arange(nlon)[:, None, None, None]
    j = np.arange(nmu)[None, :, None, None]
    a = np.arange(S)[None, None, :, None]
    b = np.arange(S)[None, None, None, :]
    l = -np.pi + 2. * np.pi * (i + (a + 0.5) / S) / nlon + 0. * (j + b)
    mu = -1. + 2. * (j + (b + 0.5) / S) / nmu + 0. * (i + a)
    st = np.sqrt(1. - mu * mu)
    d = (st * np.cos(l))[..., None] * f[0] + \
        (st * np.sin(l))[..., None] * f[1] + mu[..., None] * f[2]
    return d.reshape(nlon * nmu, S * S, 3)


def test_primary_tally_against_ray_tracing():
    """A 16^3 hydrogen-only grid, fixed cross sections, a monochromatic
    source, no re-emission, an off-centre dense blob: the primaries' tally in
    8 x 4 pixels against the mean of exp(-tau) over 16 x 16 sub-rays of each
    pixel from ionizing_optical_depths, within 5 binomial standard deviations
    plus the quadrature error (the difference to 8 x 8 sub-rays). And the
    columns of a uniform box along an axis are n x L."""
    from cmacionize_amd import GpuEngine, STROMGREN as S
    ncell, npacket, nlon, nmu = 16, 200000, 8, 4
    frame = X.tilted_frame()
    side = S["sides"][0]
    eng = GpuEngine((ncell,) * 3, S["anchor"], S["sides"], (0, 0, 0),
                    device=0)
    origin = np.array([0.05 * side, -0.03 * side, 0.02 * side])
    eng.set_sources([origin], [1.], S["luminosity"])
    eng.set_spectrum_monochromatic(S["frequency"])
    sigma = np.zeros(14)
    sigma[0] = S["sigma_H"]
    alpha = np.zeros(14)
    alpha[0] = S["alpha_H"]
    eng.set_cross_sections_fixed(sigma)
    eng.set_recombination_rates_fixed(alpha)
    assert np.array_equal(eng.cross_sections([S["frequency"]]), [sigma])
    n = ncell ** 3
    x = np.zeros((14, n))
    x[0] = 1.e-3
    # a uniform box first: N = n x_H L along the axes from the centre
    density = 3.e7
    eng.upload_cells(np.full(n, density), np.full(n, 8000.), x)
    centre = np.zeros(3)
    N = eng.ionizing_columns(centre, np.vstack([np.eye(3), -np.eye(3)]))
    assert N.shape == (6, 14)
    assert np.allclose(N[:, 0], density * 1.e-3 * 0.5 * side, rtol=1e-12,
                       atol=0.)
    assert np.all(N[:, 1:] == 0.)
    # the blob: a ball of 20 times the density off the centre
    ax = S["anchor"][0] + (np.arange(ncell) + 0.5) * (side / ncell)
    Xc, Yc, Zc = np.meshgrid(ax, ax, ax, indexing="ij")
    blob = (Xc - 0.2 * side) ** 2 + (Yc + 0.1 * side) ** 2 + \
        (Zc - 0.15 * side) ** 2 < (0.18 * side) ** 2
    shape = np.where(blob, 20., 1.).ravel()
    eng.upload_cells(shape, np.full(n, 8000.), x)
    fine = sub_rays(nlon, nmu, 16, frame)
    coarse = sub_rays(nlon, nmu, 8, frame)
    nu = [S["frequency"]]
    tau1 = eng.ionizing_optical_depths(origin, fine.reshape(-1, 3),
                                       nu)[:, 0].reshape(nlon * nmu, -1)
    tau1c = eng.ionizing_optical_depths(origin, coarse.reshape(-1, 3),
                                        nu)[:, 0].reshape(nlon * nmu, -1)
    # tau is linear in the density: the scale at which half the light escapes
    lo, hi = 0., 1.
    while np.exp(-hi * tau1).mean() > 0.5:
        hi *= 2.
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if np.exp(-mid * tau1).mean() > 0.5 else (lo, mid)
    scale = hi
    p = np.exp(-scale * tau1).mean(axis=1)
    quadrature = np.abs(p - np.exp(-scale * tau1c).mean(axis=1))
    assert 0.2 < p.mean() < 0.8
    assert p.max() > 2. * p.min()  # the blob shows
    eng.upload_cells(scale * shape, np.full(n, 8000.), x)
    # (the columns follow the state on the device)
    assert np.allclose(
        eng.ionizing_optical_depths(origin, fine[:3, 0], nu)[:, 0],
        scale * tau1[:3, 0], rtol=1e-12, atol=0.)
    eng.set_escape_tally(nlon, nmu, frame)
    eng.enable_trackers(True)
    eng.reset_grid()
    eng.shoot(23, 0, 0, npacket)
    tw, tc, _ = eng.get_counters()
    got = eng.escape_tally()
    eng.close()
    assert got[1:].sum() == 0 and got[0].sum() == tc[0]
    assert 0.2 < tc[0] / tw < 0.8
    counts = got[0, 0].ravel()
    q = p / (nlon * nmu)  # a packet is emitted into the pixel and gets out
    sigma_b = np.sqrt(npacket * q * (1. - q))
    bound = 5. * sigma_b + npacket * quadrature / (nlon * nmu)
    excess = np.abs(counts - npacket * q) / bound
    print("largest deviation / bound: %.3f; quadrature / sigma up to %.3f" %
          (excess.max(),
           (npacket * quadrature / (nlon * nmu) / sigma_b).max()))
    assert (excess <= 1.).all(), (counts, npacket * q, bound)


# 4. switches ---------------------------------------------------------------------
def stromgren_engine(ncell=16):
    from cmacionize_amd import GpuEngine, STROMGREN as S
    from test_gpu_domain import configure
    eng = GpuEngine((ncell,) * 3, S["anchor"], S["sides"], (0, 0, 0),
                    device=0)
    configure(eng, "diffuse", ncell ** 3)
    return eng


def test_switches():
    from cmacionize_amd import engine as E
    npacket = 20000
    eng = stromgren_engine()
    plain = stromgren_engine()
    with pytest.raises(E.EngineError, match="no escape tally set"):
        eng.escape_tally()
    with pytest.raises(E.EngineError, match="cmi_gpu error 3"):
        eng.reset_escape_tally()
    with pytest.raises(E.EngineError, match="orthonormal"):
        eng.set_escape_tally(4, 2, 1.001 * np.eye(3))
    with pytest.raises(E.EngineError, match="2\\^24"):
        eng.set_escape_tally(4096, 4096)
    with pytest.raises(E.EngineError, match="level bins"):
        eng._check(eng._lib.cmi_gpu_set_escape_tally(
            eng._h, 4, 2, E._p(E._f64(np.eye(3)).reshape(9)), 8, 1, 0., 0.))
    eng.set_escape_tally(6, 3, nfreq=2)
    # nothing is counted before the trackers are enabled
    eng.reset_grid()
    eng.shoot(42, 0, 0, npacket)
    assert eng.escape_tally().shape == (3, 2, 6, 3)
    assert eng.escape_tally().sum() == 0
    eng.enable_trackers(True)
    eng.reset_grid()
    eng.shoot(42, 1, 0, npacket)
    _, tc, _ = eng.get_counters()
    first = eng.escape_tally()
    assert np.array_equal(first.sum(axis=(1, 2, 3)), tc[:3]) and tc[0] > 0
    # ... and it adds up over calls until it is reset
    eng.shoot(42, 1, npacket, npacket)
    _, tc2, _ = eng.get_counters()
    assert np.array_equal(eng.escape_tally().sum(axis=(1, 2, 3)), tc2[:3])
    eng.reset_escape_tally()
    assert eng.escape_tally().sum() == 0
    eng.reset_grid()
    eng.shoot(42, 1, 0, npacket)
    assert np.array_equal(eng.escape_tally(), first)
    # disabled: the tally stands still, and the iteration is the one of an
    # engine that never had a tally
    eng.enable_trackers(False)
    for e in (eng, plain):
        e.reset_grid()
        e.shoot(42, 2, 0, npacket)
    assert np.array_equal(eng.escape_tally(), first)
    assert eng.get_counters()[0] == plain.get_counters()[0]
    assert np.array_equal(eng.get_counters()[1], plain.get_counters()[1])
    assert eng.get_counters()[2] == plain.get_counters()[2]
    J, Jp = (e.download_field(E.FIELD_MEAN_INTENSITY) for e in (eng, plain))
    # (atomics reorder the sums)
    assert np.allclose(J, Jp, rtol=1e-12, atol=0.)
    # removed
    eng.set_escape_tally(0, 0)
    with pytest.raises(E.EngineError, match="no escape tally set"):
        eng.escape_tally()
    eng.enable_trackers(True)
    eng.reset_grid()
    eng.shoot(42, 2, 0, npacket)
    assert np.array_equal(eng.get_counters()[1], plain.get_counters()[1])
    eng.close()
    plain.close()


# 5. blocks -----------------------------------------------------------------------
def test_blocks_add_up_to_the_undivided_grid():
    """The diffuse Stromgren case as 2 x 1 x 1 blocks: a hand-over is no
    escape, the blocks' tallies add up to the undivided grid's exactly."""
    from test_gpu_domain import run_pair
    frame = X.tilted_frame()
    seen = 0
    for loop, whole, (tw, tc, ns), dec, backends, driver, J, Jref in run_pair(
            "diffuse", 16, (2, 1, 1), 20000, 2):
        if loop == 0:
            for e in [whole] + [b.engine for b in backends]:
                set_tally(e, X.LINEAR_BINS, frame)
                e.enable_trackers(True)
            continue
        want = whole.escape_tally()
        parts = [b.engine.escape_tally() for b in backends]
        assert np.array_equal(want.sum(axis=(1, 2, 3)), tc[:3])
        assert np.array_equal(driver.typecount, tc)
        assert all(part.sum() > 0 for part in parts)
        assert np.array_equal(sum(parts), want)
        assert tc[0] > 0 and tc[1] > 0
        seen += 1
    assert seen == 1


# 6. the driver ---------------------------------------------------------------------
def test_cmi_gpu_writes_the_escape_tally(tmp_path):
    from test_escape_host import EXE, small_param
    from test_gpu_domain import configure
    from cmacionize_amd import GpuEngine, STROMGREN as S
    p = tmp_path / "run.param"
    p.write_text(small_param())
    r = subprocess.run([EXE, "--params", str(p)], capture_output=True,
                       text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    data = np.fromfile(tmp_path / "leak.dat")
    assert data.size == 3 * 5 * 8 * 4
    data = data.reshape(3, 5, 8, 4)
    rows = {}
    for line in open(tmp_path / "leak.txt"):
        if line.startswith("#"):
            continue
        key, _, values = line.partition(":")
        rows[key] = np.array([float(v) for v in values.split()])
    fraction = rows["total escape fraction"][0]
    assert rows["type escape fractions"].shape == (3,)
    assert rows["bin escape fractions"].shape == (5,)
    assert np.isclose(rows["type escape fractions"].sum(), fraction,
                      rtol=1e-14)
    assert np.isclose(rows["bin escape fractions"].sum(), fraction,
                      rtol=1e-14)
    eV, h = 1.6021766208e-19, 6.626070040e-34
    lo, hi = 13.6 * eV * (1. / h), 27.2 * eV * (1. / h)
    assert np.allclose(rows["bin edges (Hz)"], lo + (hi - lo) *
                       np.arange(6) / 5, rtol=1e-15)
    assert np.isclose(data.sum(), S["luminosity"] * fraction, rtol=1e-12)
    assert np.allclose(data.sum(axis=(1, 2, 3)),
                       S["luminosity"] * rows["type escape fractions"],
                       rtol=1e-12)
    # the same iteration through the Python engine: its counters
    eng = GpuEngine((16,) * 3, S["anchor"], S["sides"], (0, 0, 0), device=0)
    configure(eng, "diffuse", 16 ** 3)
    eng.reset_grid()
    eng.shoot(42, 0, 0, 20000)
    tw, tc, _ = eng.get_counters()
    eng.close()
    assert 0. < fraction < 1.
    assert fraction == tc[:3].sum() / tw
