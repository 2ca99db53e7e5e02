"""One representative call of each entry point of csrc/scatter_driver.h on
the 12^3 lexington state of tools/render_calls.py, with dust per hydrogen
nucleus and a line source: a shoot for each of the four camera kinds without
and with cube mode, the galaxy source with the single and the several-views
parallel camera, Lyman alpha with one view and with three, without and with
the radiation field - 40 000 packets each, so that every shoot crosses its
first launch and is sized at least once -, every probe kind of dust_probe and
lya_probe for the selected view 0 and for view 2, every counter getter, the
per-view counters and get_cell_source. The outputs go to an .npz; the library
is the one CMI_GPU_LIBRARY names (tools/render_calls_compare.py compares two
of them).

    python tools/scatter_calls.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import line_image_lib as L  # noqa: E402
import lyman_alpha_lib as Y  # noqa: E402
from cmacionize_amd import engine as E  # noqa: E402
from test_gpu_emissivity import random_state  # noqa: E402
from test_gpu_line_image import lexington_box  # noqa: E402
from test_gpu_physics import lexington_engine  # noqa: E402

N = 40000
SEED = 5
LINE = "HAlpha"
NCHAN, VMIN, VMAX, SIGMA_TURB = 7, -6.e4, 7.e4, 3.e3
ROWS = 300


def main():
    out = {}
    ncell = 12
    density, temperature, x = random_state(ncell, 7)
    eng = lexington_engine(ncell)
    eng.upload_cells(density, temperature, x)
    box = lexington_box(ncell)
    anchor3, sides3 = np.array(box.anchor), np.array(box.sides)
    half = 0.5 * sides3[0]
    n = ncell ** 3
    rng = np.random.default_rng(11)
    eng.set_cell_velocities(2.e4 * rng.normal(size=(3, n)))
    # an optical depth of 1 from the centre to a face at the mean density
    eng.set_dust_scattering_per_hydrogen(0.44, 0.5, 0.6,
                                         1. / (density.mean() * half))
    theta, phi = [0.7, 0.2, 2.0], [0.3, 2.5, -1.0]
    anchor, sides = L.bounding_rectangle(box, theta[0], phi[0])
    nx, ny, nlon, nlat = 20, 17, 16, 9
    r_min = sides3[0] / ncell
    origins = anchor3 + np.array([[0.3, 0.3, 0.3], [0.8, 0.4, 0.6],
                                  [1.4, 0.5, 0.5]]) * sides3
    vo = np.array([[1.e3, -2.e3, 5.e2], [0., 0., 0.], [-3.e3, 1.e3, 2.e3]])

    def put(name, value):
        if isinstance(value, dict):
            value = np.array([value[m] for m in value])
        out[name] = np.asarray(value)
        print(name, out[name].shape, float(np.nansum(out[name])), flush=True)

    cameras = {
        "parallel": lambda: eng.set_ccd_image(theta[0], phi[0], nx, ny,
                                              anchor, sides),
        "parallel_views": lambda: eng.set_ccd_images(theta, phi, nx, ny,
                                                     anchor, sides),
        "point": lambda: eng.set_sky_camera(origins[0], nlon, nlat, r_min),
        "point_views": lambda: eng.set_sky_cameras(origins, nlon, nlat,
                                                   r_min)}

    def counters(name):
        put(name + "/counters", eng.get_dust_counters())
        put(name + "/sky_counters", eng.get_sky_camera_counters())
        if eng.nviews > 1:
            put(name + "/view_counters",
                [list(eng.get_dust_view_counters(v).values())
                 for v in range(eng.nviews)])

    def unit(rows):
        return rows / np.linalg.norm(rows, axis=1)[:, None]

    def photon_rows(with_position):
        """{[pos], dir, sin theta, cos theta, phi, sin phi, cos phi, I, Q, U,
        V} of photons flying along dir"""
        d = unit(rng.normal(size=(ROWS, 3)))
        ph = np.arctan2(d[:, 1], d[:, 0])
        st = np.sqrt(1. - d[:, 2] ** 2)
        stokes = np.c_[np.ones(ROWS), rng.uniform(-0.3, 0.3, (ROWS, 3))]
        rows = np.c_[d, st, d[:, 2], ph, np.sin(ph), np.cos(ph), stokes]
        if with_position:
            pos = anchor3 + rng.uniform(0.05, 0.95, (ROWS, 3)) * sides3
            rows = np.c_[pos, rows]
        return rows

    scatter_rows = photon_rows(False)
    peel_rows = photon_rows(True)
    depth_rows = np.c_[anchor3 + rng.uniform(0., 1., (ROWS, 3)) * sides3,
                       unit(rng.normal(size=(ROWS, 3)))]

    def dust_probes(name, kinds):
        for view in (0, 2) if eng.nviews > 1 else (0,):
            eng.select_probe_view(view)
            for kind, rows, cap in kinds:
                put("%s/probe%d/view%d" % (name, kind, view),
                    eng.dust_probe(kind, SEED, 100, ROWS, rows, cap))

    common = [(E.DUST_PROBE_EMIT, None, 0),
              (E.DUST_PROBE_SCATTER, scatter_rows, 0),
              (E.DUST_PROBE_SCATTER_TOWARDS, scatter_rows, 0),
              (E.DUST_PROBE_OPTICAL_DEPTH, depth_rows, 40),
              (E.DUST_PROBE_TRACE, None, 6)]

    # the cell source: the four cameras, the image run and the cube run
    eng.set_cell_source_line(LINE)
    put("get_cell_source", np.r_[eng.get_cell_source()[0],
                                 eng.get_cell_source()[1],
                                 eng.get_cell_source()[2]])
    for kind, camera in cameras.items():
        camera()
        eng.dust_shoot(SEED, 0, N)
        put(kind + "/images", eng.download_images())
        counters(kind)
        kinds = common + [(E.DUST_PROBE_CELL_SOURCE, None, 0)]
        if kind.startswith("point"):
            kinds.append((E.DUST_PROBE_SKY_PEEL, peel_rows, 0))
        dust_probes(kind, kinds)
        eng.set_scattered_cube(
            NCHAN, VMIN, VMAX, SIGMA_TURB, observer_velocities=vo[:eng.nviews]
            if kind.startswith("point") else None)
        eng.dust_shoot(SEED, 0, N)
        put(kind + "/cube_images", eng.download_images())
        put(kind + "/cubes", eng.download_cubes())
        counters(kind + "/cube")
        dust_probes(kind + "/cube", [(E.DUST_PROBE_CUBE_TRACE, None, 6)])
        eng.set_scattered_cube(0, 0., 1.)

    # Lyman alpha: one view and three, without and with the field. H I and
    # temperature as lyman_alpha_lib.parity_scene chooses them: a line-centre
    # depth of 100 from the centre to a face
    sigma0 = Y.line_centre_cross_section(Y.doppler_width(1.0e4))
    n_HI = density / density.mean() * 100. / (sigma0 * half)
    T = np.full(n, 1.0e4)
    voigt_rows = np.c_[10. ** rng.uniform(-4., -1.7, ROWS),
                       rng.normal(0., 3., ROWS),
                       10. ** rng.uniform(-18., -12., ROWS),
                       10. ** rng.uniform(-20., -14., ROWS)]
    lya_depth_rows = np.c_[depth_rows, rng.normal(0., 4.0e4, ROWS)]
    sampler_rows = np.c_[rng.normal(0., 2.5, ROWS),
                         10. ** rng.uniform(-3.9, -1.8, ROWS)]
    for kind in ("parallel", "parallel_views"):
        cameras[kind]()
        eng.set_lyman_alpha(16, -2.e5, 2.e5, SIGMA_TURB, 0.,
                            n_HI=n_HI, temperature=T)
        for field in (False, True):
            name = "lya/%s/field%d" % (kind, field)
            eng.set_lya_field(field)
            eng.reset_lya()
            eng.lya_shoot(SEED, 0, N)
            images, cubes = eng.download_lya()
            put(name + "/images", images)
            put(name + "/cubes", cubes)
            put(name + "/counters", eng.get_lya_counters())
            if field:
                put(name + "/rows", eng.download_lya_field())
                put(name + "/spin_temperature",
                    np.array(eng.lya_spin_temperature(N, 2.725)))
        for view in (0, 2) if eng.nviews > 1 else (0,):
            eng.select_probe_view(view)
            for probe, rows, cap in ((E.LYA_PROBE_VOIGT, voigt_rows, 0),
                                     (E.LYA_PROBE_OPTICAL_DEPTH,
                                      lya_depth_rows, 0),
                                     (E.LYA_PROBE_SAMPLER, sampler_rows, 0),
                                     (E.LYA_PROBE_TRACE, None, 6)):
                put("lya/%s/probe%d/view%d" % (kind, probe, view),
                    eng.lya_probe(probe, SEED, 100, ROWS, rows, cap))
        eng.set_lyman_alpha(0, 0., 1.)
    put("lyman_alpha_emissivity", eng.lyman_alpha_emissivity())

    # the galaxy source: the single and the several-views parallel camera
    eng.set_continuous_source_spiral_galaxy(0.5 * half, 0.1 * half, 0.2)
    for kind in ("parallel", "parallel_views"):
        cameras[kind]()
        eng.dust_shoot(SEED, 0, N)
        put("galaxy/" + kind + "/images", eng.download_images())
        counters("galaxy/" + kind)
        dust_probes("galaxy/" + kind, common)
    eng.close()
    np.savez(sys.argv[1], **out)
    print("CALLS_OK", len(out))


if __name__ == "__main__":
    main()
