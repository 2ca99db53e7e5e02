"""The SPH mappings on the device (include/cmi_gpu.h, "SPH mappings";
cmacionize_amd/csrc/sph_map_kernels.h) against the numpy brute force over all
pairs of tests/sph_map_lib.py, within the derived bound

    |device - reference| <= (8 + n) 2^-53 sum_{pairs} |a_i| W(0, h_i)

per output (n contributing pairs; an output without one is exactly 0), and
the host users that opt in: the library mode's "centroid" mapping and the SPH
snapshot density functions with device mapping switched on."""
import ctypes as C
import functools
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import sph_map_lib as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cmacionize_amd", "libcmi_gpu_library.so")
CMI_GPU = os.path.join(ROOT, "cmacionize_amd", "cmi-gpu")
BENCH = os.path.join(ROOT, "benchmarks")
GOLDEN = os.path.join(ROOT, "tests", "golden")
M_H = 1.6737236e-27
KERNELS = {0: "spline_h", 1: "spline_2h"}

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def cached_case(name):
    return {"A": lambda: S.case_a(False), "B": lambda: S.case_a(True),
            "C": S.case_c}[name]()


@functools.lru_cache(maxsize=None)
def cached_pairs(name, form):
    c = cached_case(name)
    return S.Pairs(c["positions"], c["h"], form, c["grid"], c["periodic_box"])


@pytest.fixture(scope="module")
def engine():
    from cmacionize_amd import GpuEngine
    anchor, sides, ncell = S.GRID_A
    eng = GpuEngine(ncell, anchor, sides)
    yield eng
    eng.close()


def to_cells(engine, case, form, K):
    return engine.sph_map_to_cells(
        case["positions"], case["h"], case["amplitudes"][:K],
        kernel=KERNELS[form], periodic_box=case["periodic_box"],
        grid=case["grid"])


def to_particles(engine, case, form):
    return engine.sph_map_to_particles(
        case["positions"], case["h"], case["cell_values"],
        kernel=KERNELS[form], periodic_box=case["periodic_box"],
        grid=case["grid"])


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", ["A", "B"])
def test_cells_from_particles(engine, name, form, K):
    """Case A: geometry - three unequal axes, h from 0.3 to 4 cell sides,
    particles outside the grid, one on a midpoint, empty cells. Case B: the
    same grid as a periodic box, kernels across all faces and corners."""
    case = cached_case(name)
    got = to_cells(engine, case, form, K)
    assert got.shape == (K,) + tuple(case["grid"][2])
    expect, tol = cached_pairs(name, form).to_cells(case["amplitudes"][:K])
    if name == "A":
        assert (tol[0] == 0.).any()     # cells that no particle covers
    S.assert_within(got.reshape(K, -1), expect, tol,
                    "cells <- particles %s form %d K %d" % (name, form, K))
    assert engine.sph_map_stats()["declined"] == 0


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", ["A", "B"])
def test_particles_from_cells(engine, name, form):
    case = cached_case(name)
    got = to_particles(engine, case, form)
    expect, tol = cached_pairs(name, form).to_particles(case["cell_values"])
    assert (tol == 0.).any()            # particles that cover no midpoint
    S.assert_within(got, expect, tol,
                    "particles <- cells %s form %d" % (name, form))


@pytest.mark.parametrize("form,K", [(0, 1), (0, 3), (1, 3)])
def test_long_lists_run_the_chunk_loop(engine, form, K):
    """Case C: a clump of 3000 particles inside one cell makes tile lists
    longer than the staging chunk."""
    case = cached_case("C")
    got = to_cells(engine, case, form, K)
    stats = engine.sph_map_stats()
    assert stats["tiles"] == 8 * 4 * 3
    assert stats["longest_list"] > 3000 > stats["stage_chunk"] > 0
    assert stats["longest_list"] % stats["stage_chunk"] != 0   # ... a tail
    assert stats["list_entries"] >= len(case["h"])
    expect, tol = cached_pairs("C", form).to_cells(case["amplitudes"][:K])
    S.assert_within(got.reshape(K, -1), expect, tol,
                    "cells <- particles C form %d K %d" % (form, K))


@pytest.mark.parametrize("form", [0, 1])
def test_both_classes_of_particles(engine, form):
    case = cached_case("C")
    got = to_particles(engine, case, form)
    stats = engine.sph_map_stats()
    assert stats["lane_class"] > 100 and stats["wave_class"] > 100
    assert stats["lane_class"] + stats["wave_class"] <= len(case["h"])
    expect, tol = cached_pairs("C", form).to_particles(case["cell_values"])
    S.assert_within(got, expect, tol, "particles <- cells C form %d" % form)


def host_library():
    assert os.path.exists(LIB), "build() makes libcmi_gpu_library.so"
    L = C.CDLL(LIB)
    vp = C.c_void_p
    L.cmi_gpu_library_map_to_cells.argtypes = [
        C.c_char_p, C.c_int, vp, vp, vp, vp, vp, C.c_size_t, C.c_double,
        C.c_double, vp, vp, vp, vp, vp]
    L.cmi_gpu_library_map_to_particles.argtypes = [
        C.c_char_p, C.c_int, vp, vp, vp, vp, vp, C.c_size_t, C.c_double,
        C.c_double, vp, vp, vp, vp, vp, vp]
    return L


def host_arguments(case):
    anchor, sides, ncell = case["grid"]
    keep = [np.ascontiguousarray(case["positions"][:, a]) for a in range(3)]
    keep += [np.ascontiguousarray(case["h"]),
             np.ascontiguousarray(case["amplitudes"][0]),
             np.ascontiguousarray(anchor, dtype=np.float64),
             np.ascontiguousarray(sides, dtype=np.float64),
             np.array(ncell, dtype=np.int32)]
    return keep


def test_clumped_case_against_the_host_centroid_mapping(engine):
    """Case C, form 0, K = 1 against cmi_gpu_library_map_to_cells on the
    host: where a kernel covers the midpoint both are density / m_H."""
    case = cached_case("C")
    L = host_library()
    x, y, z, h, m, anchor, sides, nc = host_arguments(case)
    host = np.zeros(int(np.prod(case["grid"][2])))
    assert L.cmi_gpu_library_map_to_cells(
        b"centroid", 0, x.ctypes.data, y.ctypes.data, z.ctypes.data,
        h.ctypes.data, m.ctypes.data, len(h), 1., 1., None,
        anchor.ctypes.data, sides.ctypes.data, nc.ctypes.data,
        host.ctypes.data) == 0
    got = to_cells(engine, case, 0, 1).reshape(-1)
    _, tol = cached_pairs("C", 0).to_cells(m)
    covered = tol[0] > 0.
    assert covered.sum() > 1000
    err = np.abs(got / M_H - host)[covered]
    print("device against host centroid: worst error / bound = %.3g" %
          np.max(err / (tol[0][covered] / M_H)))
    assert np.all(err <= tol[0][covered] / M_H)
    assert np.all(got[~covered] == 0.)


def test_declines(engine):
    from cmacionize_amd.engine import SphMapDeclined
    case = cached_case("B")
    h = case["h"].copy()
    h[7] = 0.5 * case["grid"][1].min()     # twice the reach = the side
    with pytest.raises(SphMapDeclined) as info:
        engine.sph_map_to_cells(case["positions"], h, case["amplitudes"][:1],
                                periodic_box=case["periodic_box"],
                                grid=case["grid"])
    assert info.value.reason == "wide_kernel"
    assert engine.sph_map_stats()["declined"] == 2
    with pytest.raises(SphMapDeclined) as info:
        engine.sph_map_to_particles(case["positions"], h, case["cell_values"],
                                    periodic_box=case["periodic_box"],
                                    grid=case["grid"])
    assert info.value.reason == "wide_kernel"
    with pytest.raises(SphMapDeclined) as info:
        engine.sph_map_to_cells(np.zeros((0, 3)), np.zeros(0),
                                np.zeros((1, 0)), grid=case["grid"])
    assert info.value.reason == "no_particles"
    # without a periodic box nothing wraps and the same kernel is taken
    engine.sph_map_to_cells(case["positions"], h, case["amplitudes"][:1],
                            grid=case["grid"])
    assert engine.sph_map_stats()["declined"] == 0


# ------------------------------------------------------ the host users --

def test_library_chain_on_the_device(engine):
    """SPHArrayInterface::write through the device operators against the
    host's, case A with the same x_H per cell. The bound of the inverse
    operator propagated through nH_i = 1 - m_i out_i, where out_i sums
    W g_c with g_c = (1 - x_c) / cellmass_c and cellmass_c itself carries the
    forward operator's bound: |d nH_i| <= m_i (tol_i + sum_c W_ic g_c
    tol_c / cellmass_c) + 2^-52 (1 + m_i out_i)."""
    case = cached_case("A")
    L = host_library()
    x, y, z, h, m, anchor, sides, nc = host_arguments(case)
    xH = np.random.default_rng(21).uniform(0., 1., int(np.prod(nc)))
    args = [b"centroid", 0, x.ctypes.data, y.ctypes.data, z.ctypes.data,
            h.ctypes.data, m.ctypes.data, len(h), 1., 1., None,
            anchor.ctypes.data, sides.ctypes.data, nc.ctypes.data]
    host, device = np.zeros(len(h)), np.zeros(len(h))
    assert L.cmi_gpu_library_map_to_particles(
        *args, xH.ctypes.data, host.ctypes.data) == 0
    L.cmi_gpu_library_device_map_to_particles.argtypes = \
        L.cmi_gpu_library_map_to_particles.argtypes
    assert L.cmi_gpu_library_device_map_to_particles(
        *args, xH.ctypes.data, device.ctypes.data) == 0
    pairs = cached_pairs("A", 0)
    mass, mass_tol = pairs.to_cells(m)
    mass, mass_tol = mass[0], mass_tol[0]
    covered = mass > 0.
    g = np.where(covered, (1. - xH) / np.where(covered, mass, 1.), 0.)
    out, tol = pairs.to_particles(g)
    tol_g = np.where(covered, g * mass_tol / np.where(covered, mass, 1.), 0.)
    extra = np.bincount(pairs.i, weights=pairs.w * tol_g[pairs.c],
                        minlength=len(h))
    bound = m * (tol + extra) + 2. * S.EPS * (1. + m * out)
    err = np.abs(device - host)
    print("library chain: worst error / bound = %.3g" % np.max(err / bound))
    assert np.all(err <= bound)
    assert (device < 0.999).sum() > 300
    # ... and the brute force agrees with both
    assert np.all(np.abs(device - (1. - m * out)) <= bound)
    # the forward probe on the device: the host's numbers, floor included
    dens_host = np.zeros(len(xH))
    dens_dev = np.zeros(len(xH))
    L.cmi_gpu_library_device_map_to_cells.argtypes = \
        L.cmi_gpu_library_map_to_cells.argtypes
    assert L.cmi_gpu_library_map_to_cells(*args, dens_host.ctypes.data) == 0
    assert L.cmi_gpu_library_device_map_to_cells(
        *args, dens_dev.ctypes.data) == 0
    assert np.all(np.abs(dens_dev - dens_host)[covered] <=
                  mass_tol[covered] / M_H)
    assert (~covered).any()
    assert np.array_equal(dens_dev[~covered], dens_host[~covered])


def library_for_runs():
    L = host_library()
    dp = C.POINTER(C.c_double)
    fp = C.POINTER(C.c_float)
    L.cmi_init.argtypes = [C.c_char_p, C.c_int, C.c_double, C.c_double,
                           C.c_char_p, C.c_int]
    L.cmi_compute_neutral_fraction_dp.argtypes = [dp] * 6 + [C.c_size_t]
    L.cmi_compute_neutral_fraction_mp.argtypes = [dp] * 3 + [fp] * 3 + [
        C.c_size_t]
    L.cmi_gpu_library_set_device_mapping.argtypes = [C.c_int]
    L.cmi_gpu_library_device_mapping_count.restype = C.c_long
    return L


def test_library_mode_with_device_mapping_matches_the_oracle(oracle,
                                                             tmp_path):
    """The configuration and the assertions of
    test_cmi_library.test_library_mode_matches_the_oracle (16^3 cells, 16^3
    particles, 40000 packets, 6 iterations; atol 5e-3 against the oracle
    chain, the inner and outer neutral fractions) with device mapping
    switched on: both mappings of both compute calls run on the device."""
    import test_cmi_library as T
    L = library_for_runs()
    before = L.cmi_gpu_library_device_mapping_count()
    L.cmi_gpu_library_set_device_mapping(1)
    try:
        T.test_library_mode_matches_the_oracle(L, oracle, tmp_path)
    finally:
        L.cmi_gpu_library_set_device_mapping(0)
    assert L.cmi_gpu_library_device_mapping_count() - before == 2 * 3


def test_a_declined_mapping_is_the_host_path(tmp_path, capfd):
    """Kernels wider than half the particles' box: the device mapping
    declines, says so under talk, and the run is the host path's."""
    PC = 3.086e16
    side, npart_side = 10. * PC, 6
    text = open(os.path.join(BENCH, "stromgren.param")).read()
    text = text.replace("[64, 64, 64]", "[8, 8, 8]")
    text = text.replace("number of photons: 1e6", "number of photons: 20000")
    text = text.replace("number of iterations: 20", "number of iterations: 2")
    text = text.replace("type: Gadget", "type: AsciiFile")
    p = tmp_path / "lib.param"
    p.write_text(text)
    d = side / npart_side
    ax = (np.arange(npart_side) + 0.5) * d - 0.5 * side
    pos = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"),
                   axis=-1).reshape(-1, 3)
    n = len(pos)
    x, y, z = (np.ascontiguousarray(pos[:, a]) for a in range(3))
    h = np.full(n, 0.55 * side)
    m = np.full(n, 100. * 1.e6 * M_H * d ** 3)
    L = library_for_runs()
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    results = []
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        for on in (1, 0):
            L.cmi_gpu_library_set_device_mapping(on)
            nH = np.full(n, -1.)
            L.cmi_init(str(p).encode(), 1, 1., 1., b"centroid", 1)
            assert L.cmi_gpu_library_status() == 0
            L.cmi_compute_neutral_fraction_dp(ptr(x), ptr(y), ptr(z), ptr(h),
                                              ptr(m), ptr(nH), n)
            assert L.cmi_gpu_library_status() == 0
            L.cmi_destroy()
            results.append((nH, capfd.readouterr().out))
    finally:
        L.cmi_gpu_library_set_device_mapping(0)
        os.chdir(cwd)
    (with_switch, said), (without, said_nothing) = results
    # two host runs: the same mapping; the engine's atomics add the mean
    # intensities up in another order each time (the smoke test allows them
    # 1e-9 for that), which two iterations carry into nH
    assert np.allclose(with_switch, without, rtol=0., atol=1e-8), \
        np.abs(with_switch - without).max()
    assert np.all(np.isfinite(without)) and without.min() < 0.999
    assert said.count("Device mapping declined") == 2, said
    assert "on the host" in said
    assert "Device mapping" not in said_nothing


def read_binary_snapshot(path, ncell):
    blob = open(path, "rb").read()
    assert struct.unpack_from("<3q", blob) == (ncell,) * 3
    return np.frombuffer(blob, dtype="<f8", offset=24).reshape(16, -1)


def snapshot_particles(name, tmp_path):
    """positions, h, masses (SI), kernel form and the grid of a fixture"""
    if name == "Phantom":
        data = np.loadtxt(os.path.join(GOLDEN, "Phantom_data.txt")) * 0.01
        block = "  type: PhantomSnapshot\n  filename: %s" % os.path.join(
            GOLDEN, "Phantomtest.dat")
        return (data[:, :3], data[:, 3], np.full(len(data), 1.e-5), 1, block,
                ("-2.1 cm", "5.2 cm"), (-0.021, 0.052), None)
    if name == "SPHNG":
        data = np.loadtxt(os.path.join(GOLDEN, "SPHNG_data.txt"))
        block = "  type: SPHNGSnapshot\n  filename: %s" % os.path.join(
            GOLDEN, "SPHNGtest.dat")
        return (data[:, :3] * 0.01, data[:, 4] * 0.01, data[:, 3] * 0.001, 1,
                block, ("-2.1 cm", "5.2 cm"), (-0.021, 0.052), None)
    fixture = os.path.join(GOLDEN, "gadget_test.hdf5")
    cli = tmp_path / "hdf5_reader_cli"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I",
                    os.path.join(ROOT, "cmacionize_amd", "host"), "-o",
                    str(cli), os.path.join(ROOT, "tests", "support",
                                           "hdf5_reader_cli.cpp"), "-lz"],
                   check=True)

    def read(path):
        r = subprocess.run([str(cli), fixture, path], capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr
        return json.loads(r.stdout)
    units = read("/Units")["attributes"]
    ul = units["Unit length in cgs (U_L)"][0] * 0.01
    um = units["Unit mass in cgs (U_M)"][0] * 0.001
    pos = np.array(read("/PartType0/Coordinates")["data"]).reshape(-1, 3) * ul
    h = np.array(read("/PartType0/SmoothingLength")["data"]) * ul
    m = np.array(read("/PartType0/Masses")["data"]) * um
    periodic = read("/RuntimePars")["attributes"]["PeriodicBoundariesOn"][0]
    box = None
    if periodic:
        size = read("/Header")["attributes"]["BoxSize"]
        size = [size[a] if len(size) >= 3 else size[0] for a in range(3)]
        box = np.array([0., 0., 0.] + [v * ul for v in size])
    block = "  type: GadgetSnapshot\n  filename: %s" % fixture
    return pos, h, m, 0, block, ("0. m", "1. m"), (0., 1.), box


@pytest.mark.parametrize("name", ["Phantom", "SPHNG", "Gadget"])
def test_snapshot_density_functions_on_the_device(name, tmp_path):
    """cmi-gpu --dry-run-snapshot on the fixtures of tests/golden on a 20^3
    grid, with and without --device-mapping: the number density within the
    operator's bound (over m_H, plus the rounding of that division), the
    fields whose post-processing is constant exactly equal."""
    ncell = 20
    pos, h, m, form, block, (anchor_text, side_text), (anchor, side), box = \
        snapshot_particles(name, tmp_path)
    text = open(os.path.join(BENCH, "stromgren.param")).read()
    text = text.replace("[64, 64, 64]", "[%d, %d, %d]" % ((ncell,) * 3))
    text = text.replace("anchor: [-5. pc, -5. pc, -5. pc]",
                        "anchor: [%s, %s, %s]" % ((anchor_text,) * 3))
    text = text.replace("sides: [10. pc, 10. pc, 10. pc]",
                        "sides: [%s, %s, %s]" % ((side_text,) * 3))
    old = text[text.index("DensityFunction:"):]
    old = old[:old.index("\n\n")]
    text = text.replace(old, "DensityFunction:\n" + block)
    text = text.replace("type: Gadget\n", "type: Binary\n")
    assert side_text in text and block in text and "type: Binary" in text
    fields, said = {}, {}
    for label, flags in (("host", []), ("device", ["--device-mapping"])):
        d = tmp_path / label
        d.mkdir()
        (d / "run.param").write_text(text)
        r = subprocess.run([CMI_GPU, "--params", "run.param",
                            "--dry-run-snapshot"] + flags,
                           capture_output=True, text=True, cwd=str(d))
        assert r.returncode == 0, r.stderr + r.stdout
        fields[label] = read_binary_snapshot(d / "stromgren_000.bin", ncell)
        said[label] = r.stdout
    assert "onto the cells on the device" in said["device"]
    assert "device" not in said["host"]
    grid = (np.full(3, anchor), np.full(3, side), (ncell,) * 3)
    pairs = S.Pairs(pos, h, form, grid, box)
    expect, tol = pairs.to_cells(m)
    expect, tol = expect[0] / M_H, tol[0] / M_H
    host, device = fields["host"], fields["device"]
    assert (tol > 0.).sum() > 100
    # (the brute force knows the fixture's particles to 1e-14 only: good to
    # 1e-11 of the central values the bound is made of)
    assert np.all(np.abs(device[0] - expect) <= 1e-11 * tol / (8. * S.EPS))
    bound = tol + 2. * S.EPS * expect
    err = np.abs(device[0] - host[0])
    print("%s: number density, worst error / bound = %.3g" %
          (name, np.max(err[tol > 0.] / bound[tol > 0.])))
    assert np.all(err <= bound)
    # temperature (8000 K, or the file's zeros through the kernel), neutral
    # fractions 1e-6 and everything else the writer holds: equal
    assert np.array_equal(device[1:], host[1:])
    assert np.all(device[2] == 1.e-6) and np.all(device[3] == 1.e-6)
    if name != "Gadget":
        assert np.all(device[1] == 8000.)


def test_a_declined_snapshot_mapping_is_the_host_path_to_the_bit(tmp_path):
    """A periodic Gadget snapshot with one kernel as wide as half the box:
    the operator declines, cmi-gpu says so and writes what the host path
    writes, bit for bit (the host's sums are serial per cell)."""
    writer = tmp_path / "make_sph_snapshot"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I",
                    os.path.join(ROOT, "cmacionize_amd", "host"), "-o",
                    str(writer), os.path.join(ROOT, "tests", "support",
                                              "make_sph_snapshot.cpp"),
                    "-lz"], check=True)
    rng = np.random.default_rng(8)
    n, ncell, box = 600, 10, 10.
    x = rng.uniform(0., box, (n, 3))
    m = rng.uniform(0.5, 1.5, n) * 1e-3
    h = rng.uniform(0.8, 1.6, n)
    h[17] = 0.5 * box
    rho = rng.uniform(0.5, 2., n) * 1e-3
    T = rng.uniform(2000., 4000., n)
    xH = rng.uniform(0., 1., n)
    raw = tmp_path / "particles.bin"
    with open(raw, "wb") as f:
        f.write(struct.pack("<Q", n))
        for a in (x, m, h, rho, T, xH):
            f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
    subprocess.run([str(writer), str(tmp_path / "sph.hdf5"), str(raw), "1",
                    str(box), repr(3.086e18), repr(1.989e33), repr(2.5),
                    str(1 | 2 | 4 | 8)], check=True)
    text = open(os.path.join(BENCH, "stromgren.param")).read()
    text = text.replace("[64, 64, 64]", "[%d, %d, %d]" % ((ncell,) * 3))
    text = text.replace("anchor: [-5. pc, -5. pc, -5. pc]",
                        "anchor: [0. pc, 0. pc, 0. pc]")
    old = text[text.index("DensityFunction:"):]
    old = old[:old.index("\n\n")]
    text = text.replace(old, "DensityFunction:\n  type: GadgetSnapshot\n"
                        "  filename: ../sph.hdf5\n"
                        "  use neutral fraction: true")
    text = text.replace("type: Gadget\n", "type: Binary\n")
    assert "GadgetSnapshot" in text and "anchor: [0. pc" in text
    fields, said = {}, {}
    for label, flags in (("host", []), ("device", ["--device-mapping"])):
        d = tmp_path / label
        d.mkdir()
        (d / "run.param").write_text(text)
        r = subprocess.run([CMI_GPU, "--params", "run.param",
                            "--dry-run-snapshot"] + flags,
                           capture_output=True, text=True, cwd=str(d))
        assert r.returncode == 0, r.stderr + r.stdout
        fields[label] = read_binary_snapshot(d / "stromgren_000.bin", ncell)
        said[label] = r.stdout
    assert "Device mapping declined" in said["device"]
    assert "smallest side of the periodic box" in said["device"]
    assert "on the host" in said["device"]
    assert "Device mapping" not in said["host"]
    # (a cell no kernel covers has the neutral fraction 0 / 0 on both)
    assert np.array_equal(fields["device"], fields["host"], equal_nan=True)
    assert (fields["host"][0] > 0.).sum() > 900
