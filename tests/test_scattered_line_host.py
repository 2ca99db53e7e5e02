"""The CPU restatement of the scattered-light line images
(tests/support/scattered_line_reference.c) on its own, and the driver's new
keys - no GPU: the cell-luminosity source's tables and selection rule against
numpy on integer-valued weights (every sum exact), zero-weight cells never
chosen, the Monte Carlo image at albedo 0 against the ray-traced restatement
(line_image_lib.render), `cmi-gpu --emission --dry-run` with the scattering
keys."""
import os
import subprocess

import numpy as np
import pytest

import line_image_lib as L
import scattered_line_lib as S

BLOCK = S.BLOCK


_model = S.unit_model
FIELDS = S.fields()


def _boundary_draws(w, rng, n):
    """uniforms in (0, 1): random ones and ones placed to rounding on the
    cell and block boundaries of the cumulative sum"""
    cum = np.cumsum(w)
    total = cum[-1]
    edges = np.unique(np.r_[cum, cum[BLOCK - 1::BLOCK]]) / total
    near = np.concatenate([edges, np.nextafter(edges, 0.),
                           np.nextafter(edges, 2.),
                           np.nextafter(np.nextafter(edges, 0.), 0.)])
    tiny = np.nextafter(0., 1.)
    u = np.r_[rng.uniform(size=n), near, tiny, 2. ** -53, 1. - 2. ** -53]
    return u[(u > 0.) & (u < 1.)]


@pytest.mark.parametrize("name", list(FIELDS))
def test_tables_and_selection_against_numpy(name):
    ncell, w = FIELDS[name]
    ref = S.Restatement(_model(ncell), w)
    assert ref.status == 0
    total, B, Cs = ref.tables()
    n = len(w)
    nblock = (n + BLOCK - 1) // BLOCK
    pad = np.r_[w, np.zeros(nblock * BLOCK - n)].reshape(nblock, BLOCK)
    assert np.array_equal(Cs, np.cumsum(pad, axis=1).ravel()[:n])
    assert np.array_equal(B, np.cumsum(pad.sum(axis=1)))
    side = 1. / np.array(ncell, float)
    assert total == side[0] * side[1] * side[2] * w.sum()
    u = _boundary_draws(w, np.random.default_rng(8), 100000)
    assert len(u) >= 100000
    got = ref.select(u)
    t = u * B[-1]
    inside = t < B[-1]  # u B[last] can round up to B[last]
    want = np.searchsorted(np.cumsum(w), t[inside], side="right")
    assert np.array_equal(got[inside], want)
    # no zero-weight cell, whatever the rounding
    assert np.all(w[got] > 0.)
    assert np.all(got[~inside] == np.flatnonzero(w)[-1])
    # every emitting cell can be chosen
    assert set(got) == set(np.flatnonzero(w))


def test_rounded_sums_never_choose_a_dark_cell():
    """weights over 12 decades, most cells dark: the block sums round, so
    t - B[b - 1] can reach past a block's last cell sum (the rule's step 4)"""
    rng = np.random.default_rng(12)
    ncell = (10, 12, 9)
    w = 10. ** rng.uniform(-6., 6., 1080)
    w[rng.uniform(size=1080) < 0.6] = 0.
    w[BLOCK:2 * BLOCK] = 0.
    ref = S.Restatement(_model(ncell), w)
    assert ref.status == 0
    _, B, Cs = ref.tables()
    last = np.minimum(np.arange(1, len(B) + 1) * BLOCK, len(w)) - 1
    edges = np.r_[B, np.r_[0., B[:-1]] + Cs[last]] / B[-1]
    u = np.r_[rng.uniform(size=100000), edges, np.nextafter(edges, 0.),
              np.nextafter(edges, 2.), 1. - 2. ** -53]
    u = u[(u > 0.) & (u < 1.)]
    got = ref.select(u)
    assert np.all(w[got] > 0.)
    # the frequencies follow the weights: the brightest cell
    top = int(np.argmax(w))
    share = np.mean(ref.select(rng.uniform(size=100000)) == top)
    p = w[top] / w.sum()
    assert abs(share - p) < 5. * np.sqrt(p * (1. - p) / 100000)


def test_refused_fields():
    ncell = (4, 4, 4)
    for bad in (-1., np.nan, np.inf):
        w = np.ones(64)
        w[17] = bad
        assert S.Restatement(_model(ncell), w).status == 1
    assert S.Restatement(_model(ncell), np.zeros(64)).status == 2


def test_emission_of_the_restatement():
    """positions inside the chosen cell, unit directions, the cell a
    function of the first draw alone"""
    ncell, w = FIELDS["10x12x9"]
    ref = S.Restatement(_model(ncell), w)
    rows = ref.emit(42, 0, 20000)
    cell = rows[:, 0].astype(int)
    assert np.all(w[cell] > 0.)
    idx = np.stack([cell // (12 * 9), (cell // 9) % 12, cell % 9], axis=1)
    f = rows[:, 1:4] * np.array(ncell) - idx
    assert np.all(f >= 0.) and np.all(f <= 1.)
    assert 0.45 < f.mean() < 0.55
    assert np.allclose(np.linalg.norm(rows[:, 4:7], axis=1), 1., atol=1e-15)
    assert np.allclose(rows[:, 4:7].mean(axis=0), 0., atol=0.03)


def test_monte_carlo_at_albedo_0_is_the_ray_traced_image():
    """Statistical identity. At albedo 0 only the direct light reaches the
    image, and its expectation is the ray-traced image with extinction
    n sigma. Per pixel |I_mc - I_rt| <= 5 sqrt(sum of squared contributions),
    both in W m^-2 sr^-1 (the Monte Carlo image x L_total / (N A_pixel)).

    Chosen values (scattered_line_lib.identity_model): the 10 x 12 x 9 grid
    in a box of sides (2.5, 3, 2.25); view theta = 1.1, phi = 0.6, a generic
    direction under which the box's silhouette is a hexagon and the chord -
    and with it the intensity - falls to zero linearly at its edge, so that
    the ray tracer's 8 x 8 midpoint samples see no jump inside a pixel;
    sigma = 0.08 with densities of 5 .. 20, optical depths of 1 to 3 across
    the box; 4e5 packets on 16 x 16 pixels over the bounding rectangle, a
    thousand and more per pixel inside the silhouette. Pixels with fewer
    than 100 contributions (the silhouette's rim) are skipped, at most a
    quarter of the lit ones."""
    box, model, field = S.identity_model()
    ref = S.Restatement(model, field)
    assert ref.status == 0
    N = S.IDENTITY_PACKETS
    image, counters, squares, hits = ref.shoot(S.IDENTITY_SEED, 0, N, True)
    total, _, _ = ref.tables()
    scale = total / (N * model.pixel_area)
    assert counters[1] > 0 and counters[2] == 0  # they scatter, unseen
    assert not image[1].any() and not image[2].any()
    rt = L.render(box, field, model.theta, model.phi, model.nx, model.ny,
                  model.img_anchor, model.img_sides, 8,
                  extinction=model.density * model.sigma)[0]
    lit = rt > 0.
    judged = lit & (hits >= 100)
    print("lit", lit.sum(), "judged", judged.sum(), "median hits",
          np.median(hits[judged]))
    assert lit.sum() > 100
    assert judged.sum() >= 0.75 * lit.sum()
    assert np.median(hits[judged]) > 300
    assert not image[0][~lit].any()
    z = np.abs(image[0] * scale - rt)[judged] / \
        (np.sqrt(squares[judged]) * scale)
    print("worst", z.max(), "rms", np.sqrt(np.mean(z ** 2)))
    assert z.max() <= 5.
    # and it is an identity, not a loose bound: z is of order one
    assert 0.5 < np.sqrt(np.mean(z ** 2)) < 1.5


# -------------------------------------------------------------- driver --

BLOCK_TEXT = ("EmissivityValues:\n  Halpha: true\n"
              "EmissionImages:\n  view theta: 60. degrees\n"
              "  dust cross section per hydrogen: %s m^2\n")


def _emission(tmp_path, text, dry_run=True):
    params = tmp_path / "lines.param"
    params.write_text(text)
    cmd = [S.CMI_GPU, "--emission", "--params", str(params), "--file",
           str(tmp_path / "nowhere.hdf5")]
    if dry_run:
        cmd.insert(2, "--dry-run")
    r = subprocess.run(cmd, capture_output=True, text=True,
                       cwd=str(tmp_path))
    return r, str(params) + ".used-values"


def test_driver_parses_the_scattering_keys(tmp_path):
    """with every key the block is accepted (the run then fails on the
    snapshot, which does not exist); the keys and their defaults appear in
    the used-values"""
    text = BLOCK_TEXT % "2.e-27" + (
        "  scattering: true\n  number of packets: 20000\n  random seed: 7\n"
        "  dust albedo: 0.54\n  dust asymmetry: 0.44\n"
        "  dust peak linear polarisation: 0.43\n")
    r, _ = _emission(tmp_path, text)
    assert r.returncode != 0 and "Could not open" in r.stderr, r.stderr
    r, used = _emission(tmp_path, text, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    used = open(used).read()
    for word in ("scattering: true", "number of packets: 20000",
                 "random seed: 7", "dust albedo: 0.54",
                 "dust asymmetry: 0.44",
                 "dust peak linear polarisation: 0.43"):
        assert word in used, (word, used)
    # defaults; without dust the three dust keys are not needed
    r, used = _emission(tmp_path, BLOCK_TEXT % "0." + "  scattering: true\n",
                        dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    used = open(used).read()
    assert "number of packets: 1000000" in used and "random seed: 42" in used


@pytest.mark.parametrize("missing", ["dust albedo", "dust asymmetry",
                                     "dust peak linear polarisation"])
def test_driver_requires_the_dust_keys(tmp_path, missing):
    keys = {"dust albedo": 0.54, "dust asymmetry": 0.44,
            "dust peak linear polarisation": 0.43}
    text = BLOCK_TEXT % "2.e-27" + "  scattering: true\n" + "".join(
        "  %s: %r\n" % kv for kv in keys.items() if kv[0] != missing)
    r, used = _emission(tmp_path, text)
    assert r.returncode != 0
    assert missing + " is required" in r.stderr, r.stderr
    assert "Could not open" not in r.stderr
    assert not os.path.exists(used)


@pytest.mark.parametrize("line, message", [
    ("number of packets: 0", "number of packets must be positive"),
    ("dust albedo: 1.5", "dust albedo must be in [0, 1]"),
    ("dust asymmetry: 0.", "dust asymmetry must be non-zero"),
])
def test_driver_refuses_bad_scattering_values(tmp_path, line, message):
    keys = {"number of packets": 100, "dust albedo": 0.54,
            "dust asymmetry": 0.44, "dust peak linear polarisation": 0.43}
    keys.pop(line.split(":")[0])
    text = BLOCK_TEXT % "2.e-27" + "  scattering: true\n  " + line + "\n" + \
        "".join("  %s: %r\n" % kv for kv in keys.items())
    r, _ = _emission(tmp_path, text)
    assert r.returncode != 0 and message in r.stderr, r.stderr


def test_driver_without_scattering_reads_none_of_the_new_keys(tmp_path):
    """a key that is read appears in the used-values with its default: none
    of the new ones does, with the switch absent or false"""
    new = ("scattering", "number of packets", "random seed", "albedo",
           "asymmetry", "polarisation")
    r, used = _emission(tmp_path, BLOCK_TEXT % "2.e-27", dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    absent = open(used).read()
    assert "EmissionImages:" in absent
    for word in new:
        assert word not in absent, word
    r, used = _emission(tmp_path,
                        BLOCK_TEXT % "2.e-27" + "  scattering: false\n",
                        dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    off = open(used).read()
    for word in new[1:]:
        assert word not in off, word
    # the switch itself is not counted as read either
    assert "scattering: value not used" in off
    assert [l for l in off.split("\n") if "scattering" not in l] == \
        absent.split("\n")
