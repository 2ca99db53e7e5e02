"""CPU tests of the escape maps: the binning function the kernels call (run on
the host), the plain-C restatement of the tally on the oracle, and the
EscapeTally: block of the .param driver."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import escape_lib as X  # noqa: E402
from bench_inputs import bench_text  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cmacionize_amd", "cmi-gpu")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cmacionize_amd",
                                                   "csrc")], check=True)
        subprocess.run(["make", "-C", os.path.join(ROOT, "cmacionize_amd",
                                                   "host")], check=True)
    return EXE


# the binning function --------------------------------------------------------
def unit(l, mu, frame):
    """the unit vector of longitude l and d . e_3 = mu in `frame`"""
    f = np.asarray(frame, dtype=np.float64)
    st = np.sqrt(1. - mu * mu)
    return st * np.cos(l) * f[0] + st * np.sin(l) * f[1] + mu * f[2]


def test_escape_pixels_known_answers():
    from cmacionize_amd import engine as E
    nlon, nmu = 12, 6
    I = np.eye(3)
    pix = E.escape_pixels([I[0]], nlon, nmu)
    assert pix[0] // nmu == nlon // 2       # d = e_1: l = 0
    assert pix[0] % nmu == nmu // 2         # mu = 0: an edge, the upper pixel
    assert E.escape_pixels([I[2]], nlon, nmu)[0] % nmu == nmu - 1
    assert E.escape_pixels([-I[2]], nlon, nmu)[0] % nmu == 0
    # l = -pi: atan2 of the smallest negative y (a -0. does not survive the
    # sum of the three products) at x = -1
    assert np.arctan2(-5e-324, -1.) == -np.pi
    assert E.escape_pixels([[-1., -5e-324, 0.]], nlon, nmu)[0] // nmu == 0
    # l = +pi: the upper end of the range belongs to the last pixel
    assert E.escape_pixels([[-1., 0., 0.]], nlon, nmu)[0] // nmu == nlon - 1
    # odd numbers of pixels: e_1 sits in the middle pixel, not on an edge
    assert E.escape_pixels([I[0]], 5, 3)[0] == 2 * 3 + 1
    # e_2: l = pi / 2 is the edge between pixels 8 and 9 of 12
    assert E.escape_pixels([I[1]], nlon, nmu)[0] // nmu == 9


def test_escape_pixels_edges_go_to_the_upper_pixel():
    from cmacionize_amd import engine as E
    # mu edges that are exact in binary: nmu = 8, mu = -1 + k / 4, in the
    # plane l = 0 of the identity frame (d . e_3 = mu exactly)
    nmu = 8
    for k in range(1, nmu):
        mu = -1. + k / 4.
        d = [np.sqrt(1. - mu * mu), 0., mu]
        assert E.escape_pixels([d], 4, nmu)[0] % nmu == k
        # (the formula's mu + 1 rounds to an ulp of 1: step by a few of them)
        below = [d[0], 0., mu - 4. * np.finfo(np.float64).eps]
        assert E.escape_pixels([below], 4, nmu)[0] % nmu == k - 1
    # l edges at multiples of pi / 2, nlon = 4: the axes themselves
    for k, d in enumerate([[-1., -5e-324, 0.], [0., -1., 0.], [1., 0., 0.],
                           [0., 1., 0.]]):
        assert E.escape_pixels([d], 4, 2)[0] // 2 == k


def test_escape_pixels_tilted_frame_and_centres():
    from cmacionize_amd import engine as E
    frame = X.tilted_frame()
    assert np.allclose(frame @ frame.T, np.eye(3), atol=1e-15)
    nlon, nmu = 12, 6
    # every pixel's centre lies in its pixel, and so do points well inside
    centres = E.escape_pixel_centres(nlon, nmu, frame)
    assert centres.shape == (nlon, nmu, 3)
    assert np.allclose((centres ** 2).sum(axis=2), 1., atol=1e-15)
    pix = E.escape_pixels(centres.reshape(-1, 3), nlon, nmu, frame)
    assert np.array_equal(pix, np.arange(nlon * nmu))
    for i in range(nlon):
        for j in range(nmu):
            l = -np.pi + 2. * np.pi * (i + 0.3) / nlon
            mu = -1. + 2. * (j + 0.8) / nmu
            assert E.escape_pixels([unit(l, mu, frame)], nlon, nmu,
                                   frame)[0] == i * nmu + j
    # the frame's own axes
    assert E.escape_pixels([frame[0]], nlon, nmu, frame)[0] // nmu == nlon // 2
    assert E.escape_pixels([frame[2]], nlon, nmu, frame)[0] % nmu == nmu - 1
    assert E.escape_pixels([-frame[2]], nlon, nmu, frame)[0] % nmu == 0
    # random directions: the library, the restatement and numpy agree
    rng = np.random.default_rng(5)
    d = rng.normal(size=(20000, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    ref, dist = X.numpy_pixels(d, nlon, nmu, frame)
    far = dist > X.EDGE_MARGIN
    assert far.all()
    assert np.array_equal(E.escape_pixels(d, nlon, nmu, frame), ref)
    assert np.array_equal(X.reference_pixels(d, nlon, nmu, frame), ref)
    # equal areas: every pixel gets its share of isotropic directions
    counts = np.bincount(ref, minlength=nlon * nmu)
    assert counts.min() > 0.7 * len(d) / (nlon * nmu)


def test_escape_pixels_refuses_bad_arguments():
    from cmacionize_amd import engine as E
    skew = [[1., 0., 0.], [1e-6, 1., 0.], [0., 0., 1.]]
    with pytest.raises(E.EngineError, match="orthonormal"):
        E.escape_pixels([[1., 0., 0.]], 12, 6, skew)
    with pytest.raises(E.EngineError, match="orthonormal"):
        E.escape_pixel_centres(12, 6, 2. * np.eye(3))
    with pytest.raises(E.EngineError):
        E.escape_pixels([[1., 0., 0.]], 0, 6)
    with pytest.raises(E.EngineError):
        E.escape_pixel_centres(12, 0)


def test_escape_map_and_spectrum_normalisation():
    from cmacionize_amd import engine as E
    rng = np.random.default_rng(1)
    tally = rng.integers(0, 5, size=(3, 4, 8, 2)).astype(np.float64)
    totweight = 2. * tally.sum()
    fmap = E.escape_fraction_map(tally, totweight)
    assert fmap.shape == (8, 2)
    # its mean over the equal-area pixels is the escape fraction
    assert np.isclose(fmap.mean(), 0.5, rtol=1e-14)
    spec = E.escape_spectrum(tally, totweight, 4.e49)
    assert spec.shape == (3, 4)
    assert np.isclose(spec.sum(), 2.e49, rtol=1e-14)


# the restatement ---------------------------------------------------------------
@pytest.mark.parametrize("bins", [X.LINEAR_BINS, X.LEVEL_BINS],
                         ids=["linear", "level"])
def test_restatement_on_lexington(oracle, bins):
    """The restatement's packet loop is cmio_shoot's: same counters, same
    integrals; per type the tally sums to typecount[0..2] (weights are 1);
    and with this seed no escaped packet lies within 1e-9 of an edge, which
    is what the GPU parity tests rely on."""
    frame = X.tilted_frame()
    ref = X.lexington_copy()
    ref.shoot(X.LEX_SEED, 1, 0, X.LEX_PACKETS)
    sim = X.lexington_copy()
    sky, tw, tc, edge = X.shoot(sim, X.LEX_SEED, 1, 0, X.LEX_PACKETS, X.NLON,
                                X.NMU, frame, bins)
    assert tw == ref.totweight == X.LEX_PACKETS
    assert np.array_equal(tc, ref.typecount)
    for ion in range(14):
        assert np.allclose(sim.J[ion], ref.J[ion], rtol=1e-12, atol=0.)
    assert sky.shape == (3, bins[1], X.NLON, X.NMU)
    assert np.array_equal(sky.sum(axis=(1, 2, 3)), tc[:3])
    assert tc[0] > 0 and tc[1] > 0 and tc[2] > 0 and tc[3] > 0
    assert np.array_equal(sky, np.round(sky))
    assert edge[0] > X.EDGE_MARGIN, edge
    assert edge[1] > X.EDGE_MARGIN, edge
    # more than one bin and every pixel are in use
    assert (sky.sum(axis=(0, 2, 3)) > 0).sum() > 1
    assert (sky.sum(axis=(0, 1)) > 0).all()


def test_restatement_on_the_periodic_box(oracle):
    """The periodic Stromgren case (x and y periodic: packets leave through
    z only): the counters are cmio_shoot's, the tally sums to them, and no
    escaped packet lies within 1e-9 of an edge."""
    sim, _ = X.periodic_simulation()
    ref, _ = X.periodic_simulation()
    ref.shoot(X.PERIODIC_SEED, 0, 0, X.PERIODIC_PACKETS)
    sky, tw, tc, edge = X.shoot(sim, X.PERIODIC_SEED, 0, 0,
                                X.PERIODIC_PACKETS, X.NLON, X.NMU,
                                np.eye(3), X.LINEAR_BINS)
    assert tw == ref.totweight == X.PERIODIC_PACKETS
    assert np.array_equal(tc, ref.typecount)
    assert np.array_equal(sky.sum(axis=(1, 2, 3)), tc[:3])
    assert tc[0] > 0 and tc[1] > 0 and tc[3] > 0
    assert edge[0] > X.EDGE_MARGIN and edge[1] > X.EDGE_MARGIN, edge


# the driver ----------------------------------------------------------------------
ESCAPE_BLOCK = """EscapeTally:
  number of longitude pixels: 8
  number of mu pixels: 4
  frame pole: [0.3, -0.5, 0.8]
  frame zero longitude: [0.9, 0.2, 0.1]
  output name: leak
  FrequencyBins:
    type: Linear
    number of bins: 5
    minimum frequency: 13.6 eV
    maximum frequency: 27.2 eV
"""


def small_param(extra=ESCAPE_BLOCK):
    text = bench_text("stromgren_diffuse.param")
    text = text.replace("[64, 64, 64]", "[16, 16, 16]")
    text = text.replace("number of photons: 1e6", "number of photons: 20000")
    text = text.replace("number of iterations: 20", "number of iterations: 1")
    text = text.replace("type: Gadget", "type: AsciiFile")
    return text + extra


def test_escape_block_is_read_and_described(exe, tmp_path):
    from cmacionize_amd.engine import sky_frame
    p = tmp_path / "run.param"
    p.write_text(small_param())
    r = subprocess.run([exe, "--params", str(p), "--dry-run", "--describe"],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)["escape_tally"]
    assert d["nlon"] == 8 and d["nmu"] == 4 and d["nfreq"] == 5
    assert d["bins"] == "Linear" and d["output_name"] == "leak"
    # eV -> Hz as the reference converts (src/UnitConverter.hpp:156-159,271)
    eV, h = 1.6021766208e-19, 6.626070040e-34
    assert d["minimum_frequency"] == 13.6 * eV * (1. / h) / 1.
    assert d["maximum_frequency"] == 27.2 * eV * (1. / h) / 1.
    frame = sky_frame((0.3, -0.5, 0.8), (0.9, 0.2, 0.1))
    assert np.allclose(np.reshape(d["frame"], (3, 3)), frame, rtol=0.,
                       atol=1e-15)
    # a dry run with output dumps the keys
    r = subprocess.run([exe, "--params", str(p), "--dry-run",
                        "--dry-run-snapshot"],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    used = open(str(p) + ".used-values").read()
    assert "EscapeTally:" in used
    assert "number of longitude pixels: 8" in used
    assert "number of mu pixels: 4" in used
    assert "output name: leak" in used
    assert "number of bins: 5" in used
    # without the block: no key in the description, none in the dump
    q = tmp_path / "plain.param"
    q.write_text(small_param(""))
    r = subprocess.run([exe, "--params", str(q), "--dry-run", "--describe"],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert "escape_tally" not in json.loads(r.stdout)
    subprocess.run([exe, "--params", str(q), "--dry-run",
                    "--dry-run-snapshot"], check=True, capture_output=True,
                   cwd=str(tmp_path))
    assert "EscapeTally" not in open(str(q) + ".used-values").read()


@pytest.mark.parametrize("old,new,message", [
    ("number of longitude pixels: 8", "number of longitude pixels: 0",
     "EscapeTally"),
    ("number of mu pixels: 4", "number of mu pixels: -2", "EscapeTally"),
    ("number of longitude pixels: 8", "number of longitude pixels: 3000000",
     "2^24"),
    ("type: Linear", "type: Logarithmic", "Unknown FrequencyBins type"),
    ("frame zero longitude: [0.9, 0.2, 0.1]",
     "frame zero longitude: [0.6, -1., 1.6]", "parallel"),
])
def test_escape_block_errors(exe, tmp_path, old, new, message):
    p = tmp_path / "bad.param"
    assert old in ESCAPE_BLOCK
    p.write_text(small_param(ESCAPE_BLOCK.replace(old, new)))
    r = subprocess.run([exe, "--params", str(p), "--dry-run"],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
