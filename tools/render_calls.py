"""One representative call of each entry point of csrc/render_driver.h on a
12^3 lexington state: more lines / fields than one batch, more channels than
one block, and the continuum's chunk loops past one chunk. The outputs go to
an .npz; the library is the one CMI_GPU_LIBRARY names
(tools/render_calls_compare.py compares two of them).

    python tools/render_calls.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import line_image_lib as L  # noqa: E402
from cmacionize_amd import engine as E  # noqa: E402
from test_gpu_emissivity import random_state  # noqa: E402
from test_gpu_line_image import LEX_LINES, lexington_box  # noqa: E402
from test_gpu_physics import lexington_engine  # noqa: E402


def main():
    out = {}
    ncell = 12
    density, temperature, x = random_state(ncell, 7)
    eng = lexington_engine(ncell)
    eng.upload_cells(density, temperature, x)
    box = lexington_box(ncell)
    n = ncell ** 3
    rng = np.random.default_rng(11)
    lines = list(LEX_LINES)                                    # 11: 7 + 4
    ions = [m for m in LEX_LINES if m in E.LINE_ATOMIC_WEIGHTS]  # 10
    vel = 2.e4 * rng.normal(size=(3, n))
    eng.set_cell_velocities(vel)
    fields = 10. ** rng.uniform(-2., 1., (9, n))
    widths = 10. ** rng.uniform(3., 4.5, (9, n))
    k = 10. ** rng.uniform(-18.5, -16.5, n)
    theta, phi, s = 0.7, 0.3, 2
    anchor, sides = L.bounding_rectangle(box, theta, phi)
    nx, ny, nchan = 40, 33, 19
    vmin, vmax = -6.e4, 7.e4
    sigma = 2.e-27
    origin = box.anchor + 0.3 * box.sides
    d = rng.normal(size=(3000, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    vo = np.array([1.e3, -2.e3, 5.e2])
    nu = 10. ** np.linspace(8., 11., 19)
    bg = E.planck_function(nu, 2.725)

    def put(name, value):
        if isinstance(value, dict):
            value = np.array([value[m] for m in value])
        out[name] = np.asarray(value)
        print(name, out[name].shape, float(np.nansum(out[name])), flush=True)

    put("render_line_images", eng.render_line_images(
        lines, theta, phi, nx, ny, anchor, sides, s, sigma))
    put("render_field_images", eng.render_field_images(
        fields, theta, phi, nx, ny, anchor, sides, s, extinction=k))
    xy = anchor + sides * rng.uniform(-0.1, 1.1, (500, 2))
    put("line_image_probe", eng.line_image_probe(theta, phi, xy, 40))
    put("render_line_cube", eng.render_line_cube(
        ions, theta, phi, nx, ny, anchor, sides, nchan, vmin, vmax, s, sigma,
        3.e3))
    put("render_field_cube", eng.render_field_cube(
        fields, widths, theta, phi, nx, ny, anchor, sides, nchan, vmin, vmax,
        s, extinction=k, velocity=vel))
    put("render_line_sky", eng.render_line_sky(lines, origin, d, sigma))
    put("render_field_sky", eng.render_field_sky(fields, origin, d,
                                                 extinction=k))
    put("sky_probe", eng.sky_probe(origin, d[:500], 40))
    put("sky_map_directions", E.sky_map_directions(37, 21)[0])
    put("render_line_sky_map", eng.render_line_sky_map(
        lines, origin, 37, 21, dust_cross_section=sigma))
    put("render_line_sky_cube", eng.render_line_sky_cube(
        ions, origin, d, nchan, vmin, vmax, sigma, 3.e3, vo))
    put("render_field_sky_cube", eng.render_field_sky_cube(
        fields, widths, origin, d, nchan, vmin, vmax, extinction=k,
        velocity=vel, observer_velocity=vo))
    put("render_line_sky_map_cube", eng.render_line_sky_map_cube(
        ions, origin, 37, 21, nchan, vmin, vmax, dust_cross_section=sigma,
        sigma_turb=3.e3, observer_velocity=vo))
    kappa, source = eng.free_free_coefficients(nu)
    put("free_free_coefficients", np.array([kappa, source]))
    put("render_continuum_images", eng.render_continuum_images(
        nu, theta, phi, nx, ny, anchor, sides, s, background=bg))
    put("render_field_continuum_images", eng.render_field_continuum_images(
        kappa, source, theta, phi, nx, ny, anchor, sides, s, background=bg))
    put("render_continuum_sky", eng.render_continuum_sky(nu, origin, d,
                                                         background=bg))
    put("render_field_continuum_sky", eng.render_field_continuum_sky(
        kappa, source, origin, d, background=bg))
    put("render_continuum_sky_map", eng.render_continuum_sky_map(
        nu, origin, 37, 21, background=bg))
    put("continuum_probe_parallel", eng.continuum_probe(
        kappa[:5], source[:5], xy, 40, theta=theta, phi=phi,
        background=bg[:5]))
    put("continuum_probe_point", eng.continuum_probe(
        kappa[:5], source[:5], d[:500], 40, origin=origin, background=bg[:5]))
    # the absorbing line cubes: the 21-cm client and the caller's fields
    put("render_hi_cube", eng.render_hi_cube(
        theta, phi, nx, ny, anchor, sides, nchan, vmin, vmax, s, 3.e3,
        background_temperature=2.725))
    put("render_hi_sky_cube", eng.render_hi_sky_cube(
        origin, d, nchan, vmin, vmax, 3.e3, background_temperature=2.725,
        observer_velocity=vo))
    put("render_hi_sky_map_cube", eng.render_hi_sky_map_cube(
        origin, 37, 21, nchan, vmin, vmax, sigma_turb=3.e3,
        observer_velocity=vo))
    hi = eng.hi_coefficients(3.e3)
    put("hi_coefficients", hi)
    put("render_field_absorbing_cube", eng.render_field_absorbing_cube(
        hi["a"], hi["sl"], hi["b"], theta, phi, nx, ny, anchor, sides, nchan,
        vmin, vmax, s, velocity=vel, kc=hi["kc"], sc=hi["sc"],
        background=hi["sl"].mean()))
    put("render_field_absorbing_sky_cube",
        eng.render_field_absorbing_sky_cube(
            hi["a"], hi["sl"], hi["b"], origin, d, nchan, vmin, vmax,
            velocity=vel, kc=hi["kc"], sc=hi["sc"],
            background=hi["sl"].mean(), observer_velocity=vo))
    put("absorbing_cube_probe_parallel", eng.absorbing_cube_probe(
        hi["a"], hi["sl"], hi["b"], xy, 40, 5, vmin, vmax, theta=theta,
        phi=phi, velocity=vel, kc=hi["kc"], sc=hi["sc"],
        background=hi["sl"].mean()))
    put("absorbing_cube_probe_point", eng.absorbing_cube_probe(
        hi["a"], hi["sl"], hi["b"], d[:500], 40, 5, vmin, vmax,
        origin=origin, velocity=vel, kc=hi["kc"], sc=hi["sc"],
        background=hi["sl"].mean(), observer_velocity=vo))
    # the chunk loops past one chunk, through the continuum's launch size
    eng.set_tuning(continuum_launch_rays=1000)
    put("render_continuum_images_chunked", eng.render_continuum_images(
        nu, theta, phi, nx, ny, anchor, sides, s, background=bg))
    put("render_continuum_sky_chunked", eng.render_continuum_sky(
        nu, origin, d, background=bg))
    eng.close()
    np.savez(sys.argv[1], **out)
    print("CALLS_OK", len(out))


if __name__ == "__main__":
    main()
