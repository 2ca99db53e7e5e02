"""Several cameras per Monte Carlo run: K parallel views
(cmi_gpu_set_ccd_images) or K point observers (cmi_gpu_set_sky_cameras) share
the packets' walk; each view's image is the single camera's.

The scene is test_gpu_scattered_line.py's: the 10 x 12 x 9 identity grid at
albedo 0.6, a 24 x 24 image or a 24 x 12 map, 30 000 packets, 3 views.

Tolerances. An addend of view v is the single camera's addend (the same
device functions, the same expressions); only the order in which the atomics
add them differs. test_additive's tolerance for exactly that - rtol 1e-12,
atol 1e-14 of the largest |I| - is used wherever two device images are
compared. Against the CPU restatements the scheme is test_whole_run's: rtol
1e-9 per pixel, culprit packets traced and shown to be threshold cases."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import line_image_lib as L
import scattered_line_lib as S
import scattered_sky_lib as K
import test_gpu_dust as D
import test_gpu_scattered_sky as TS
from test_gpu_dust import SEED, _bad_pixels, _culprits

pytestmark = pytest.mark.gpu

ALBEDO = 0.6
N = 30000
KINDS = ("parallel", "point")
MAX_VIEWS = 64  # CMI_GPU_MAX_VIEWS
ENOMEM = 4  # include/cmi_gpu.h


def _close(a, b):
    """test_additive's tolerance: equal addends summed in another order"""
    return np.allclose(a, b, rtol=1e-12, atol=1e-14 * np.abs(b[0]).max())


class Parallel:
    """three parallel views: IDENTITY_VIEW; along the z axis (sin theta ==
    0); one whose anchor and sides are a part of its bounding rectangle, so
    that events fall outside the image"""
    shape = (24, 24)

    def __init__(self):
        self.box, self.model, self.field = S.identity_model(ALBEDO, 24, 24)
        m = self.model
        a1, s1 = L.bounding_rectangle(self.box, 0., 0.)
        a2, s2 = L.bounding_rectangle(self.box, 2.0, -1.3)
        a2 = (a2[0] + 0.2 * s2[0], a2[1] + 0.3 * s2[1])
        s2 = (0.5 * s2[0], 0.6 * s2[1])
        self.views = [(m.theta, m.phi, tuple(m.img_anchor), tuple(m.img_sides)),
                      (0., 0., tuple(a1), tuple(s1)),
                      (2.0, -1.3, a2, s2)]
        assert np.sin(self.views[1][0]) == 0.
        # far off the model: nothing lands in it
        self.off = (m.theta, m.phi, (m.img_anchor[0] + 100., m.img_anchor[1]),
                    tuple(m.img_sides))

    def set_views(self, eng, views):
        eng.set_ccd_images([v[0] for v in views], [v[1] for v in views], 24,
                           24, [v[2] for v in views], [v[3] for v in views])

    def set_single(self, eng, view):
        eng.set_ccd_image(view[0], view[1], 24, 24, view[2], view[3])

    def view_model(self, view):
        m = self.model
        return S.Model(m.anchor, m.sides, m.ncell, m.density, m.sigma,
                       m.albedo, m.g, m.p_l, view[0], view[1], 24, 24, view[2],
                       view[3])

    def restatement(self, view):
        return S.Restatement(self.view_model(view), self.field)

    def is_threshold_case(self, view, ref, gt, ct, cap):
        return D._is_threshold_case(self.view_model(view).describe(), ref, gt,
                                    ct, cap)

    def single_counters(self, eng):
        return {"nexcluded": 0, "noutside": 0}


class Point:
    """three observers of one full-sky 24 x 12 map: IDENTITY_OBSERVER with
    the pole along z (Q, U not rotated); one outside the box; one with a
    tilted pole (Q, U rotated)"""
    shape = (24, 12)
    window = (K.FULL_LON, K.FULL_LAT)

    def __init__(self):
        self.box, self.model, self.field = S.identity_model(ALBEDO, 24, 24)
        self.views = [
            (K.IDENTITY_OBSERVER, K.IDENTITY_FRAME, 0.25),
            ((2.6, 1.1, 5.3), K.IDENTITY_FRAME, 0.),
            ((-0.2, 1.4, 2.9), TS.TILTED, 0.05)]
        # outside the box, beyond +z, with the pole towards +z: the box lies
        # at latitudes below 0 and the window of `away` above 0.5
        self.away = (K.FULL_LON, (0.5, 1.4))
        self.off = ((0.3, 2.1, 9.), K.IDENTITY_FRAME, 0.)

    def set_views(self, eng, views, window=None):
        lon, lat = window or self.window
        eng.set_sky_cameras([v[0] for v in views], 24, 12,
                            [v[2] for v in views], lon, lat,
                            [v[1] for v in views])

    def camera(self, view, window=None):
        lon, lat = window or self.window
        return K.Camera(view[0], 24, 12, view[2], lon, lat, view[1])

    def set_single(self, eng, view, window=None):
        self.camera(view, window).apply(eng)

    def restatement(self, view):
        return K.Restatement(self.model, self.field, self.camera(view))

    def is_threshold_case(self, view, ref, gt, ct, cap):
        return TS._is_threshold_case(self.model.describe(), self.camera(view),
                                     ref, gt, ct, cap)

    def single_counters(self, eng):
        return eng.get_sky_camera_counters()


SETUPS = {"parallel": Parallel, "point": Point}


@pytest.fixture(scope="module")
def scenes():
    """per kind: the setup, one engine, the K-view run of [0, N) with its
    counters, and each view's single-camera run on the same engine"""
    out = {}
    engines = []
    for kind in KINDS:
        s = SETUPS[kind]()
        eng = S.make_engine(s.model, s.field)
        engines.append(eng)
        s.set_views(eng, s.views)
        eng.dust_shoot(SEED, 0, N)
        run = {"images": eng.download_images(),
               "counters": eng.get_dust_counters(),
               "sky": eng.get_sky_camera_counters(),
               "views": [eng.get_dust_view_counters(v) for v in range(3)],
               "single": []}
        for view in s.views:
            s.set_single(eng, view)
            eng.dust_shoot(SEED, 0, N)
            run["single"].append({"image": eng.download_image(),
                                  "counters": eng.get_dust_counters(),
                                  "sky": s.single_counters(eng)})
        out[kind] = (s, eng, run)
    yield out
    for eng in engines:
        eng.close()


class _View:
    """one view of an engine with several, for test_gpu_dust._culprits"""

    def __init__(self, eng, view):
        self.eng, self.view = eng, view

    def reset_image(self):
        self.eng.reset_image()

    def dust_shoot(self, *args):
        self.eng.dust_shoot(*args)

    def download_image(self):
        return self.eng.download_image_view(self.view)


# ------------------------------ 1. each view is the single camera's image --

@pytest.mark.parametrize("kind", KINDS)
def test_each_view_is_the_single_cameras_image(scenes, kind):
    s, eng, run = scenes[kind]
    multi = run["images"]
    assert multi.shape == (3, 3) + s.shape
    c = run["counters"]
    assert c["npackets"] == N and c["ncapped"] == 0
    walks = []
    for v, single in enumerate(run["single"]):
        image, sc = single["image"], single["counters"]
        assert np.count_nonzero(image[0]) > 20
        assert np.abs(image[1]).max() > 0. and np.abs(image[2]).max() > 0.
        print(kind, v, "largest difference / largest I",
              np.abs(multi[v] - image).max() / np.abs(image[0]).max())
        assert _close(multi[v], image), v
        assert sc["npackets"] == c["npackets"] == N
        assert sc["nscatter"] == c["nscatter"]
        vc = run["views"][v]
        walks.append(sc["nsteps"] - vc["nsteps"])
        assert vc["natomics"] == sc["natomics"], v
        assert vc["nexcluded"] == single["sky"]["nexcluded"], v
        assert vc["noutside"] == single["sky"]["noutside"], v
    # the views differ ...
    assert not _close(multi[1], multi[0]) and not _close(multi[2], multi[0])
    # ... the walk does not
    assert walks[0] > 0 and walks[1] == walks[0] and walks[2] == walks[0]
    assert c["nsteps"] == walks[0] + sum(vc["nsteps"] for vc in run["views"])
    assert c["natomics"] == sum(vc["natomics"] for vc in run["views"])
    assert run["sky"] == {
        "nexcluded": sum(vc["nexcluded"] for vc in run["views"]),
        "noutside": sum(vc["noutside"] for vc in run["views"])}
    if kind == "point":
        # the exclusion radius and the rotation are per view
        assert run["views"][0]["nexcluded"] > 0
        assert run["views"][1]["nexcluded"] == 0


# ------------------------------------ 2. parity with the CPU restatement --

@pytest.mark.parametrize("kind", KINDS)
def test_whole_run_per_view(scenes, kind):
    """test_whole_run's scheme for every view of the one K-view run"""
    from cmacionize_amd import engine as E
    s, eng, run = scenes[kind]
    s.set_views(eng, s.views)
    for v, view in enumerate(s.views):
        ref = s.restatement(view)
        gpu = run["images"][v]
        cpu, cc = ref.shoot(SEED, 0, N)
        assert cc[2] == 0 and cc[3] == 0
        assert np.count_nonzero(cpu[0]) > 20 and cc[1] > N
        bad = _bad_pixels(gpu, cpu)
        print(kind, v, "differing pixels", int(bad.sum()))
        if not np.any(bad):
            assert run["counters"]["nscatter"] == cc[1]
            assert run["single"][v]["counters"]["nsteps"] == cc[0]
            if kind == "point":
                assert run["views"][v]["nexcluded"] == cc[4]
                assert run["views"][v]["noutside"] == cc[5]
            continue
        one = _View(eng, v)
        culprits = []
        _culprits(one, ref, 0, N, bad, culprits)
        assert culprits, "differing pixels without a differing packet"
        cap = 4096
        eng.select_probe_view(v)
        for k in culprits:
            gt = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, k, 1, None, cap)[0]
            ct = ref.trace(SEED, k, 1, cap)[0]
            assert s.is_threshold_case(view, ref, gt, ct, cap), (v, k)
        eng.select_probe_view(0)
        ok = np.ones(N, bool)
        ok[culprits] = False
        gpu2 = np.zeros_like(gpu)
        cpu2 = np.zeros_like(cpu)
        edges = np.flatnonzero(np.diff(np.r_[0, ok.astype(int), 0]))
        for lo, hi in zip(edges[0::2], edges[1::2]):
            eng.reset_image()
            eng.dust_shoot(SEED, int(lo), int(hi - lo))
            gpu2 += one.download_image()
            cpu2 += ref.shoot(SEED, int(lo), int(hi - lo))[0]
        assert not np.any(_bad_pixels(gpu2, cpu2))


# ------------------- 3. additive; a packet alone is the packet among others --

@pytest.mark.parametrize("kind", KINDS)
def test_additive(scenes, kind):
    s, eng, run = scenes[kind]
    a = 12345
    s.set_views(eng, s.views)
    eng.dust_shoot(SEED, 0, a)
    eng.dust_shoot(SEED, a, N - a)
    parts = eng.download_images()
    c = eng.get_dust_counters()
    assert c["ncapped"] == 0 and c["npackets"] == N
    assert c == run["counters"]
    assert [eng.get_dust_view_counters(v) for v in range(3)] == run["views"]
    for v in range(3):
        assert _close(parts[v], run["images"][v]), v


@pytest.mark.parametrize("kind", KINDS)
def test_a_packet_alone_is_the_packet_among_others(scenes, kind):
    """the guard of DESIGN.md 4.6 with several views selected, for a view
    other than 0; the rows are the single camera's rows for that view"""
    from cmacionize_amd import engine as E
    s, eng, run = scenes[kind]
    cap = 64
    s.set_single(eng, s.views[2])
    single = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, 0, 64, None, cap)
    s.set_views(eng, s.views)
    first = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, 0, 64, None, cap)
    eng.select_probe_view(2)
    among = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, 0, 64, None, cap)
    assert among[:, 1].max() >= 2
    assert np.array_equal(among, single)
    assert not np.array_equal(among, first)
    for k in (0, 1, 17, 31, 32, 63, int(np.argmax(among[:, 1]))):
        alone = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, k, 1, None, cap)[0]
        assert np.array_equal(alone, among[k]), k
    if kind == "point":
        # SKY_PEEL follows the selected observer too
        rng = np.random.default_rng(17)
        rows = np.zeros((200, 15))
        rows[:, 0:3] = s.model.anchor + \
            rng.uniform(size=(200, 3)) * s.model.sides
        rows[:, 3:15] = D._rows(200, 6, True)
        got = eng.dust_probe(E.DUST_PROBE_SKY_PEEL, SEED, 0, len(rows), rows)
        s.set_single(eng, s.views[2])
        want = eng.dust_probe(E.DUST_PROBE_SKY_PEEL, SEED, 0, len(rows), rows)
        assert np.array_equal(got, want)
    # a camera that is set starts at view 0 again
    s.set_views(eng, s.views)
    again = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, 0, 64, None, cap)
    assert np.array_equal(again, first)


# --------------------------------- 4. views do not leak into each other --

@pytest.mark.parametrize("kind", KINDS)
def test_views_do_not_leak(scenes, kind):
    s, eng, run = scenes[kind]
    # two identical views
    s.set_views(eng, [s.views[2], s.views[0], s.views[2]])
    eng.dust_shoot(SEED, 0, N)
    images = eng.download_images()
    assert _close(images[0], images[2])
    assert _close(images[0], run["images"][2])
    assert _close(images[1], run["images"][0])
    assert eng.get_dust_view_counters(0) == eng.get_dust_view_counters(2)
    # K = 1 through the new call is the existing call
    s.set_views(eng, [s.views[1]])
    eng.dust_shoot(SEED, 0, N)
    images = eng.download_images()
    assert images.shape == (1, 3) + s.shape
    assert _close(images[0], run["single"][1]["image"])
    assert np.array_equal(eng.download_image(), images[0])
    c = eng.get_dust_counters()
    assert c == run["single"][1]["counters"]


def test_a_parallel_view_off_the_model_stays_zero(scenes):
    s, eng, run = scenes["parallel"]
    s.set_views(eng, [s.views[0], s.off, s.views[2]])
    eng.dust_shoot(SEED, 0, N)
    images = eng.download_images()
    assert not images[1].any()
    assert eng.get_dust_view_counters(1)["natomics"] == 0
    assert eng.get_dust_view_counters(1)["nsteps"] > 0
    assert _close(images[0], run["images"][0])
    assert _close(images[2], run["images"][2])


def test_an_observer_looking_away_stays_zero(scenes):
    """a window (shared by the views) that for the observer beyond the box
    holds no part of it; the observers inside see the model through it"""
    s, eng, run = scenes["point"]
    views = [s.views[0], s.off, s.views[2]]
    s.set_views(eng, views, s.away)
    eng.dust_shoot(SEED, 0, N)
    images = eng.download_images()
    assert not images[1].any()
    vc = eng.get_dust_view_counters(1)
    assert vc["natomics"] == 0 and vc["nexcluded"] == 0
    assert vc["noutside"] > N
    for v in (0, 2):
        s.set_single(eng, views[v], s.away)
        eng.dust_shoot(SEED, 0, N)
        single = eng.download_image()
        assert np.count_nonzero(single[0]) > 0
        assert _close(images[v], single), v


# ---------------------------------------------- 5. selection and refusals --

def _raw_ccd_images(lib, eng, views, nviews=None):
    th = S._f64([v[0] for v in views])
    ph = S._f64([v[1] for v in views])
    a = S._f64([v[2] for v in views])
    sd = S._f64([v[3] for v in views])
    return lib.cmi_gpu_set_ccd_images(
        eng._h, len(views) if nviews is None else nviews, S._p(th), S._p(ph),
        24, 24, S._p(a), S._p(sd))


def _raw_sky_cameras(lib, eng, views, nviews=None):
    o = S._f64([v[0] for v in views])
    f = S._f64([v[1] for v in views])
    r = S._f64([v[2] for v in views])
    return lib.cmi_gpu_set_sky_cameras(
        eng._h, len(views) if nviews is None else nviews, S._p(o), S._p(f),
        -np.pi, np.pi, -0.5 * np.pi, 0.5 * np.pi, 24, 12, S._p(r), 1)


@pytest.mark.parametrize("kind", KINDS)
def test_selection_and_refusals(scenes, kind):
    from cmacionize_amd import engine as E
    lib = E.load_library()
    assert E.MAX_VIEWS == MAX_VIEWS
    s, eng, run = scenes[kind]
    raw = _raw_ccd_images if kind == "parallel" else _raw_sky_cameras
    n = 5000

    def image_of(apply):
        apply()
        eng.dust_shoot(SEED, 0, n)
        return eng.download_image()

    single = image_of(lambda: s.set_single(eng, s.views[2]))
    # refused calls leave the single camera and its image
    many = [s.views[0]] * (MAX_VIEWS + 1)
    assert raw(lib, eng, many, 0) == S.EINVAL
    assert b"views" in lib.cmi_gpu_last_error()
    assert raw(lib, eng, many) == S.EINVAL
    assert b"views" in lib.cmi_gpu_last_error()
    if kind == "parallel":
        bad = (0.3, 0.2, (0., 0.), (1., -1.))
    else:
        bad = (K.IDENTITY_OBSERVER, K.IDENTITY_FRAME, 0.)  # in the box, r = 0
    assert raw(lib, eng, [s.views[0], bad, s.views[2]]) == S.EINVAL
    assert b"view 1" in lib.cmi_gpu_last_error()
    if kind == "point":
        assert b"exclusion radius" in lib.cmi_gpu_last_error()
    assert np.array_equal(eng.download_image(), single)
    assert lib.cmi_gpu_download_image_view(eng._h, 1, None, None, None) == \
        S.EINVAL
    assert lib.cmi_gpu_get_dust_view_counters(
        eng._h, 0, (E.C.c_uint64 * 4)()) == S.ESTATE
    eng.reset_image()
    eng.dust_shoot(SEED, 0, n)
    assert _close(eng.download_image(), single)
    # a stack that does not fit (64 x 3 x 2^28 doubles: 412 GB)
    if kind == "parallel":
        th = S._f64(np.zeros(MAX_VIEWS))
        a = S._f64(np.zeros((MAX_VIEWS, 2)))
        sd = S._f64(np.ones((MAX_VIEWS, 2)))
        before = eng.download_image()
        assert lib.cmi_gpu_set_ccd_images(
            eng._h, MAX_VIEWS, S._p(th), S._p(th), 1 << 14, 1 << 14, S._p(a),
            S._p(sd)) == ENOMEM
        assert b"does not fit" in lib.cmi_gpu_last_error()
        assert np.array_equal(eng.download_image(), before)
        eng.reset_image()
        eng.dust_shoot(SEED, 0, n)
        assert _close(eng.download_image(), single)
    # the full number of views is accepted
    assert raw(lib, eng, many[:MAX_VIEWS]) == 0
    eng.dust_shoot(SEED, 0, 200)
    assert eng.download_image_view(MAX_VIEWS - 1)[0].sum() > 0.
    # several views, the single camera again, and the reverse
    several = image_of(lambda: s.set_views(eng, s.views))
    assert eng.nviews == 3
    assert lib.cmi_gpu_download_image_view(eng._h, 3, None, None, None) == \
        S.EINVAL
    assert lib.cmi_gpu_download_image_view(eng._h, -1, None, None, None) == \
        S.EINVAL
    assert lib.cmi_gpu_select_probe_view(eng._h, 3) == S.EINVAL
    assert lib.cmi_gpu_get_dust_view_counters(
        eng._h, 3, (E.C.c_uint64 * 4)()) == S.EINVAL
    view2 = eng.download_image_view(2)
    assert _close(view2, single)
    # a refused call leaves the views and their images too
    assert raw(lib, eng, [bad]) == S.EINVAL
    assert b"view 0" in lib.cmi_gpu_last_error()
    assert np.array_equal(eng.download_image_view(2), view2)
    back = image_of(lambda: s.set_single(eng, s.views[2]))
    assert eng.nviews == 1 and _close(back, single)
    again = image_of(lambda: s.set_views(eng, s.views))
    assert _close(again, several)
    # the other kind of camera replaces these views
    if kind == "parallel":
        K.Camera(K.IDENTITY_OBSERVER, 24, 12, 0.25).apply(eng)
    else:
        eng.set_ccd_image(0.3, 0.2, 8, 8, (-9., -9.), (18., 18.))
    eng.dust_shoot(SEED, 0, 200)
    assert eng.download_image()[0].sum() > 0.


def test_sky_cameras_serve_the_cell_source_only():
    from cmacionize_amd import GpuEngine
    from cmacionize_amd import engine as E
    lib = E.load_library()
    g = GpuEngine((8, 8, 8), (-1., -1., -1.), (2., 2., 2.), (0, 0, 0),
                  device=0)
    g.upload_cells(np.ones(512), np.zeros(512), None)
    g.set_dust_scattering_per_hydrogen(0.4, 0.3, 0.5, 0.3)
    g.set_continuous_source_spiral_galaxy(0.5, 0.1, 0.2)
    g.set_sky_cameras([(0.1, 0.2, 0.3), (3., 0., 0.)], 8, 4, [0.1, 0.])
    assert lib.cmi_gpu_dust_shoot(g._h, SEED, 0, 10) == S.ESTATE
    assert b"cell source" in lib.cmi_gpu_last_error()
    # the galaxy has several parallel views
    g.set_ccd_images([0.7, 0.], [0.3, 0.], 8, 8, (-2., -2.), (4., 4.))
    g.dust_shoot(SEED, 0, 2000)
    both = g.download_images()
    g.set_ccd_image(0., 0., 8, 8, (-2., -2.), (4., 4.))
    g.dust_shoot(SEED, 0, 2000)
    assert both[0][0].sum() > 0. and _close(both[1], g.download_image())
    g.close()


def test_galaxy_with_views_past_the_first_launch():
    """The galaxy's several-views instantiation through the chunk loop of
    cmi_gpu_dust_shoot past its first launch of 2^14 packets (the scenes above
    cross it with the cell source): [0, n) in one call against [0, 2^14) and
    [2^14, n) in two. The counters are equal, the images differ by the order
    of the atomics."""
    from cmacionize_amd import GpuEngine
    first = 1 << 14
    n = first + 100
    g = GpuEngine((8, 8, 8), (-1., -1., -1.), (2., 2., 2.), (0, 0, 0),
                  device=0)
    g.upload_cells(np.ones(512), np.zeros(512), None)
    g.set_dust_scattering_per_hydrogen(0.4, 0.3, 0.5, 0.3)
    g.set_continuous_source_spiral_galaxy(0.5, 0.1, 0.2)
    g.set_ccd_images([0.7, 0.], [0.3, 0.], 16, 16, (-2., -2.), (4., 4.))

    def result():
        return (g.download_images(), g.get_dust_counters(),
                [g.get_dust_view_counters(v) for v in range(2)])

    g.dust_shoot(SEED, 0, n)
    whole, c, views = result()
    g.reset_image()
    g.dust_shoot(SEED, 0, first)
    g.dust_shoot(SEED, first, n - first)
    parts, cp, viewsp = result()
    g.close()
    assert c["npackets"] == n and c["nscatter"] > 0
    assert cp == c and viewsp == views
    for v in range(2):
        assert whole[v][0].sum() > 0.
        assert _close(parts[v], whole[v]), v


# ------------------------------------------------------ 6. end to end --

def _line_engine(model):
    """the identity grid with a state that emits H-alpha"""
    from cmacionize_amd import GpuEngine
    from test_gpu_physics import LEX
    eng = GpuEngine(tuple(int(v) for v in model.ncell), tuple(model.anchor),
                    tuple(model.sides), (0, 0, 0), device=0)
    eng.set_abundances(LEX[1:])
    x = np.full((14, model.n), 0.3)
    x[0] = 1e-3
    eng.upload_cells(model.density, np.full(model.n, 8000.), x)
    return eng


def test_render_scattered_line_images_with_two_views():
    s = Parallel()
    m = s.model
    eng = _line_engine(m)
    lines = ["HAlpha", "OIII_5007"]
    views = [s.views[0], s.views[2]]
    tail = (N, 9, m.sigma, ALBEDO, m.g, m.p_l)
    both = eng.render_scattered_line_images(
        lines, [v[0] for v in views], [v[1] for v in views], 24, 24,
        [v[2] for v in views], [v[3] for v in views], *tail)
    assert both.shape == (2, 2, 3, 24, 24)
    for v, view in enumerate(views):
        one = eng.render_scattered_line_images(lines, view[0], view[1], 24,
                                               24, view[2], view[3], *tail)
        assert one.shape == (2, 3, 24, 24)
        for k in range(2):
            assert np.abs(one[k, 1]).max() > 0.
            assert _close(both[k, v], one[k]), (k, v)
    eng.close()


def test_render_scattered_line_sky_map_with_two_observers():
    s = Point()
    m = s.model
    eng = _line_engine(m)
    lines = ["HAlpha", "OIII_5007"]
    views = [s.views[0], s.views[2]]
    poles = [v[1][2] for v in views]
    zeros = [v[1][0] for v in views]
    radii = [v[2] for v in views]
    both = eng.render_scattered_line_sky_map(
        lines, [v[0] for v in views], 24, 12, N, 9, m.sigma, ALBEDO, m.g,
        m.p_l, radii, frame_pole=poles, frame_zero_longitude=zeros)
    assert both.shape == (2, 2, 3, 24, 12)
    for v, view in enumerate(views):
        one = eng.render_scattered_line_sky_map(
            lines, view[0], 24, 12, N, 9, m.sigma, ALBEDO, m.g, m.p_l,
            radii[v], frame_pole=poles[v], frame_zero_longitude=zeros[v])
        assert one.shape == (2, 3, 24, 12)
        for k in range(2):
            assert np.abs(one[k, 1]).max() > 0.
            assert _close(both[k, v], one[k]), (k, v)
    eng.close()


def _same_terms(got, want):
    """two driver images of the same terms, added in another order by the
    atomics (test_driver_writes_the_scattered_images' comparison)"""
    top = np.abs(want).max()
    assert top > 0.
    return np.allclose(got, want, rtol=1e-12, atol=1e-14 * top)


def test_emission_driver_writes_every_view(tmp_path):
    """`cmi-gpu --emission` on the 14^3 snapshot of the existing driver
    tests, images and sky maps at once: with `number of views: 2` /
    `number of observers: 2` the view-0 files are those of a run without
    the key and the _view1 files those of a run whose view 0 is that view"""
    exe = S.CMI_GPU
    bench = os.path.join(S.ROOT, "benchmarks")
    ncell = 14
    text = open(os.path.join(bench, "lexingtonHII40.param")).read()
    text = text.replace("[64, 64, 64]", "[%d, %d, %d]" % ((ncell,) * 3))
    text = text.replace("number of photons: 1e8", "number of photons: 30000")
    text = text.replace("number of iterations: 20", "number of iterations: 6")
    text = text.replace("NumberDensity: 0", "NumberDensity: 1")
    shutil.copy(os.path.join(bench, "lexingtonHII40.yml"), tmp_path)
    (tmp_path / "run.param").write_text(text)
    r = subprocess.run([exe, "--params", "run.param"], capture_output=True,
                       text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    snapshot = str(tmp_path / "lexingtonHII40_006.hdf5")

    nx, ny, nlon, nlat = 24, 20, 24, 12
    views = [(1.05, 0.5, -1.75e17, 3.5e17), (0., 0., -1.6e17, 3.2e17)]
    observers = [((5.e16, -3.e16, 2.e16), (0., 0., 2.), 2.e16),
                 ((-4.e16, 1.e16, 2.5e17), (1., 0., 1.), 1.e16)]

    def image_keys(view, n=""):
        return ("  view theta%s: %r radians\n  view phi%s: %r radians\n"
                "  anchor x%s: %r m\n  sides x%s: %r m\n" %
                (n, view[0], n, view[1], n, view[2], n, view[3]))

    def sky_keys(o, n=""):
        return ("  observer position%s: [%r m, %r m, %r m]\n"
                "  frame pole%s: [%r, %r, %r]\n  exclusion radius%s: %r m\n" %
                ((n,) + o[0] + (n,) + o[1] + (n, o[2])))

    dust = ("  dust cross section per hydrogen: 2e-27 m^2\n"
            "  scattering: true\n  number of packets: 20000\n"
            "  random seed: 9\n  dust albedo: 0.54\n  dust asymmetry: 0.44\n"
            "  dust peak linear polarisation: 0.43\n  output folder: %s\n" %
            str(tmp_path))

    def params(name, image_block, sky_block):
        (tmp_path / (name + ".param")).write_text(
            "EmissivityValues:\n  Halpha: true\n  OIII_5007: true\n"
            "EmissionImages:\n  image width: %d\n  image height: %d\n"
            "  anchor y: -1.5e17 m\n  sides y: 3.25e17 m\n"
            "  filename prefix: %s_image\n" % (nx, ny, name) + dust +
            image_block +
            "EmissionSkyMaps:\n  number of longitude pixels: %d\n"
            "  number of latitude pixels: %d\n  filename prefix: %s_sky\n" %
            (nlon, nlat, name) + dust + sky_block)
        copy = str(tmp_path / (name + ".hdf5"))
        shutil.copy(snapshot, copy)
        r = subprocess.run([exe, "--emission", "--params", name + ".param",
                            "--file", copy], capture_output=True, text=True,
                           cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr

    params("one", image_keys(views[0]), sky_keys(observers[0]))
    params("other", image_keys(views[1]), sky_keys(observers[1]))
    params("both",
           image_keys(views[0]) + "  number of views: 2\n" +
           image_keys(views[1], " 1"),
           sky_keys(observers[0]) + "  number of observers: 2\n" +
           sky_keys(observers[1], " 1"))
    assert not [n for n in os.listdir(tmp_path)
                if "_view" in n and not n.startswith("both_")]
    for kind, shape in (("image", (nx, ny)), ("sky", (nlon, nlat))):
        for line in ("Halpha", "OIII_5007"):
            for tag, single in (("", "one"), ("_view1", "other")):
                got = tmp_path / ("both_%s_%s%s.dat" % (kind, line, tag))
                want = tmp_path / ("%s_%s_%s.dat" % (single, kind, line))
                # the ray-traced map: the same call
                assert got.read_bytes() == want.read_bytes(), got
                polarised = False
                for stokes in "IQU":
                    got = np.fromfile(str(tmp_path / (
                        "both_%s_%s%s_scattered_%s.dat" %
                        (kind, line, tag, stokes)))).reshape(shape)
                    want = np.fromfile(str(tmp_path / (
                        "%s_%s_%s_scattered_%s.dat" %
                        (single, kind, line, stokes)))).reshape(shape)
                    scale = np.fromfile(str(tmp_path / (
                        "%s_%s_%s_scattered_I.dat" %
                        (single, kind, line)))).reshape(shape)
                    top = np.abs(scale).max()
                    assert top > 0.
                    assert np.allclose(got, want, rtol=1e-12,
                                       atol=1e-14 * top), (kind, line, tag,
                                                           stokes)
                    polarised |= stokes != "I" and np.abs(want).max() > 0.
                assert polarised
    # the views differ
    a = np.fromfile(str(tmp_path / "both_image_Halpha_scattered_I.dat"))
    b = np.fromfile(str(tmp_path / "both_image_Halpha_view1_scattered_I.dat"))
    assert not np.allclose(a, b, rtol=1e-3, atol=0.)


def test_dust_driver_writes_every_view(tmp_path):
    """`cmi-gpu --dusty-radiative-transfer` on the 32^3 fixture with a
    second view (the galaxy face-on, in a smaller image): view 0's file is
    the file of a run without the key, view 1's that of a run whose view 0
    is that view"""
    text = open(os.path.join(S.HERE, "golden", "dust",
                             "test_dustsimulation.param")).read()
    second = {"view theta": "0. degrees", "view phi": "30. degrees",
              "anchor x": "-8. kpc", "sides x": "16. kpc"}
    other = text
    for key, old in (("view theta", "89.7 degrees"), ("view phi", "0 degrees"),
                     ("anchor x", "-12.1 kpc"), ("sides x", "24.2 kpc")):
        line = "  %s: %s\n" % (key, old)
        assert line in other
        other = other.replace(line, "  %s: %s\n" % (key, second[key]))
    both = text + "CCDImage:\n  number of views: 2\n" + "".join(
        "  %s 1: %s\n" % kv for kv in second.items())
    images = {}
    for name, content in (("one", text), ("other", other), ("both", both)):
        folder = tmp_path / name
        folder.mkdir()
        (folder / "dust.param").write_text(content)
        r = subprocess.run([S.CMI_GPU, "--dusty-radiative-transfer",
                            "--params", "dust.param"], capture_output=True,
                           text=True, cwd=str(folder))
        assert r.returncode == 0, r.stderr
        images[name] = np.fromfile(
            str(folder / "test_dustsimulation_output.dat"))
        assert images[name].size == 200 * 200
    assert sorted(n for n in os.listdir(tmp_path / "both")
                  if n.endswith(".dat")) == [
        "test_dustsimulation_output.dat",
        "test_dustsimulation_output_view1.dat"]
    assert not (tmp_path / "one" / "test_dustsimulation_output_view1.dat"
                ).exists()
    view1 = np.fromfile(str(tmp_path / "both" /
                            "test_dustsimulation_output_view1.dat"))
    assert _same_terms(images["both"], images["one"])
    assert _same_terms(view1, images["other"])
    assert not np.allclose(view1, images["one"], rtol=1e-3, atol=0.)
