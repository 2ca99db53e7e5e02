"""The drivers' keys for several views per Monte Carlo run,
without a GPU: `cmi-gpu --dusty-radiative-transfer --dry-run --describe` with
`CCDImage:number of views`, and `cmi-gpu --emission` with
`EmissionImages:number of views` / `EmissionSkyMaps:number of observers` up
to the point where it opens the snapshot (which does not exist: the block is
parsed, and without --dry-run the used-values are written, before that).

tests/golden/multi_view/ holds what the drivers wrote for files without the
new keys before those existed: test_dustsimulation.describe.json and
.usedvalues.param (tests/golden/dust/test_dustsimulation.param) and
one_view_lines.param with its .usedvalues."""
import json
import math
import os
import shutil
import subprocess

import pytest

import dust_lib
import scattered_line_lib as S

GOLDEN = os.path.join(S.HERE, "golden", "multi_view")
TEST32 = os.path.join(S.HERE, "golden", "dust", "test_dustsimulation.param")
KPC = 3.086e19
MAX_VIEWS = 64  # CMI_GPU_MAX_VIEWS


# ------------------------------------------------------ the dust driver --

def _dust(tmp_path, more):
    """describe TEST32 with `more` appended; (returncode, JSON or None,
    stderr, used-values or None)"""
    path = tmp_path / "views.param"
    path.write_text(open(TEST32).read() + more)
    r = subprocess.run([dust_lib.CMI_GPU, "--dusty-radiative-transfer",
                        "--dry-run", "--describe", "--params", str(path)],
                       capture_output=True, text=True, cwd=str(tmp_path))
    used = tmp_path / "dust-parameters-usedvalues.param"
    return (r.returncode, json.loads(r.stdout) if r.returncode == 0 else None,
            r.stdout + r.stderr, used.read_text() if used.exists() else None)


THREE_VIEWS = ("CCDImage:\n  number of views: 3\n"
               "  view theta 1: 30. degrees\n  view phi 1: 10. degrees\n"
               "  view theta 2: 0. degrees\n  view phi 2: 45. degrees\n"
               "  anchor x 2: -6. kpc\n  sides y 2: 12. kpc\n")


def test_dust_driver_describes_the_views(tmp_path):
    """--dry-run --describe on a three-view file: parsing, the defaults of
    the per-view keys, the output names, the used values"""
    rc, d, text, used = _dust(tmp_path, THREE_VIEWS)
    assert rc == 0, text
    img = d["image"]
    views = d["views"]
    assert len(views) == 3
    # view 0 is today's keys
    assert views[0] == {"theta": img["theta"], "phi": img["phi"],
                        "anchor": img["anchor"], "sides": img["sides"],
                        "filename": "test_dustsimulation_output"}
    # view 1: its angles, view 0's anchor and sides
    assert views[1]["theta"] == pytest.approx(math.radians(30.), rel=1e-15)
    assert views[1]["phi"] == pytest.approx(math.radians(10.), rel=1e-15)
    assert views[1]["anchor"] == img["anchor"]
    assert views[1]["sides"] == img["sides"]
    assert views[1]["filename"] == "test_dustsimulation_output_view1"
    # view 2: one anchor and one side of its own, the others view 0's
    assert views[2]["theta"] == 0.
    assert views[2]["phi"] == pytest.approx(math.radians(45.), rel=1e-15)
    assert views[2]["anchor"] == [pytest.approx(-6. * KPC, rel=1e-15),
                                  img["anchor"][1]]
    assert views[2]["sides"] == [img["sides"][0],
                                 pytest.approx(12. * KPC, rel=1e-15)]
    assert views[2]["filename"] == "test_dustsimulation_output_view2"
    for word in ("number of views: 3", "view theta 1: 0.523599 radians",
                 "view phi 1:", "view theta 2:", "view phi 2:",
                 "anchor x 2: -1.8516e+20 m", "sides y 2: 3.7032e+20 m"):
        assert word in used, (word, used)
    # a key that was not given was not read
    for word in ("anchor x 1", "anchor y 2", "sides x 2"):
        assert word not in used, word


def test_dust_driver_without_the_key_is_as_it_was(tmp_path):
    """a file without the new keys describes, and lists as used, exactly
    what it did before they existed"""
    path = tmp_path / "test_dustsimulation.param"
    shutil.copy(TEST32, path)
    r = subprocess.run([dust_lib.CMI_GPU, "--dusty-radiative-transfer",
                        "--dry-run", "--describe", "--params", str(path)],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    want = open(os.path.join(GOLDEN,
                             "test_dustsimulation.describe.json")).read()
    assert r.stdout == want
    used = (tmp_path / "dust-parameters-usedvalues.param").read_text()
    assert used == open(os.path.join(
        GOLDEN, "test_dustsimulation.usedvalues.param")).read()
    # one view named explicitly: the same description
    rc, d, text, used = _dust(tmp_path, "CCDImage:\n  number of views: 1\n")
    assert rc == 0 and d == json.loads(want), text
    assert "number of views: 1" in used


@pytest.mark.parametrize("more, message", [
    ("CCDImage:\n  number of views: 2\n  view phi 1: 0. degrees\n",
     "CCDImage:view theta 1 is required"),
    ("CCDImage:\n  number of views: 2\n  view theta 1: 0. degrees\n",
     "CCDImage:view phi 1 is required"),
    ("CCDImage:\n  number of views: 3\n  view theta 1: 0. degrees\n"
     "  view phi 1: 0. degrees\n  view theta 2: 0. degrees\n",
     "CCDImage:view phi 2 is required"),
    ("CCDImage:\n  number of views: 0\n", "number of views must be 1..64"),
    ("CCDImage:\n  number of views: %d\n" % (MAX_VIEWS + 1),
     "number of views must be 1..64"),
])
def test_dust_driver_parameter_errors(tmp_path, more, message):
    rc, d, text, used = _dust(tmp_path, more)
    assert rc == 1 and message in text, text


# -------------------------------------------------- the emission driver --

def _emission(tmp_path, text, dry_run=True):
    """tests/test_scattered_line_host.py's helper"""
    params = tmp_path / "lines.param"
    params.write_text(text)
    used = str(params) + ".used-values"
    if os.path.exists(used):
        os.remove(used)
    cmd = [S.CMI_GPU, "--emission", "--params", str(params), "--file",
           str(tmp_path / "nowhere.hdf5")]
    if dry_run:
        cmd.insert(2, "--dry-run")
    r = subprocess.run(cmd, capture_output=True, text=True,
                       cwd=str(tmp_path))
    return r, used


ONE_VIEW = open(os.path.join(GOLDEN, "one_view_lines.param")).read()
IMAGES, SKY = ONE_VIEW.split("EmissionSkyMaps:\n")
SKY = "EmissionSkyMaps:\n" + SKY
MORE_IMAGES = ("  number of views: 3\n"
               "  view theta 1: 10. degrees\n  view phi 1: 0. degrees\n"
               "  view theta 2: 90. degrees\n  view phi 2: 90. degrees\n"
               "  anchor y 2: -2.e17 m\n  sides x 2: 3.e17 m\n")
MORE_SKY = ("  number of observers: 3\n"
            "  observer position 1: [0. m, 0. m, 9.e16 m]\n"
            "  observer position 2: [-2.e16 m, 0. m, 0. m]\n"
            "  frame pole 2: [1., 0., 0.]\n"
            "  frame zero longitude 2: [0., 0., 1.]\n"
            "  exclusion radius 2: 5.e15 m\n")


def test_emission_driver_without_the_keys_is_as_it_was(tmp_path):
    r, used = _emission(tmp_path, ONE_VIEW, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    assert open(used).read() == open(os.path.join(
        GOLDEN, "one_view_lines.param.usedvalues")).read()


def test_emission_driver_parses_the_views(tmp_path):
    """--dry-run on a file with three views and three observers gets as far
    as the snapshot; without --dry-run the used-values list the new keys and
    none that the file does not have"""
    text = IMAGES + MORE_IMAGES + SKY + MORE_SKY
    r, used = _emission(tmp_path, text)
    assert r.returncode != 0 and "Could not open" in r.stderr, r.stderr
    assert not os.path.exists(used)
    r, used = _emission(tmp_path, text, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    used = open(used).read()
    for word in ("number of views: 3", "view theta 1: 0.174533 radians",
                 "view phi 1: 0 radians", "view theta 2: 1.5708 radians",
                 "view phi 2: 1.5708 radians", "anchor y 2: -2e+17 m",
                 "sides x 2: 3e+17 m", "number of observers: 3",
                 "observer position 1: [0 m, 0 m, 9e+16 m]",
                 "observer position 2: [-2e+16 m, 0 m, 0 m]",
                 "frame pole 2: [1, 0, 0]",
                 "frame zero longitude 2: [0, 0, 1]",
                 "exclusion radius 2: 5e+15 m"):
        assert word in used, (word, used)
    assert "value not used" not in used
    for word in ("anchor x 1", "sides y 2", "frame pole 1",
                 "exclusion radius 1"):
        assert word not in used, word
    # the rest is what the one-view file lists
    new = ("number of views", "number of observers", " 1:", " 2:")
    rest = [l for l in used.split("\n") if not any(w in l for w in new)]
    assert rest == open(os.path.join(
        GOLDEN, "one_view_lines.param.usedvalues")).read().split("\n")


def test_emission_driver_reads_the_exclusion_radii_with_scattering_only(
        tmp_path):
    """like the exclusion radius itself: without the switch the per-observer
    radii are not read"""
    sky = SKY.replace("  scattering: true\n", "")
    r, used = _emission(tmp_path, IMAGES + sky + MORE_SKY, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    used = open(used).read()
    assert "observer position 2: [-2e+16 m, 0 m, 0 m]" in used
    assert "exclusion radius 2: value not used" in used


# what the two blocks read with the same code: the least of each block, the
# keys of the scattered light and a velocity axis
BLOCKS = {
    "EmissionImages": "EmissionImages:\n  view theta: 60. degrees\n",
    "EmissionSkyMaps": ("EmissionSkyMaps:\n"
                        "  observer position: [1.e16 m, 2.e16 m, -3.e16 m]\n"
                        "  exclusion radius: 1.e16 m\n"),
}
SCATTERING = ("  dust cross section per hydrogen: 2.e-27 m^2\n"
              "  scattering: true\n  number of packets: 20000\n"
              "  random seed: 7\n  dust albedo: 0.54\n  dust asymmetry: 0.44\n"
              "  dust peak linear polarisation: 0.43\n")
SCATTERING_KEYS = ("scattering", "number of packets", "random seed",
                   "dust albedo", "dust asymmetry",
                   "dust peak linear polarisation")
CHANNELS = ("  velocity channels: 4\n  velocity minimum: -10. km s^-1\n"
            "  velocity maximum: 10. km s^-1\n")


def _without(key):
    return "".join(l + "\n" for l in SCATTERING.split("\n")
                   if l and not l.startswith("  %s:" % key))


# (what follows the block's first lines, the message after "<block>:")
SHARED_ERRORS = [
    (SCATTERING.replace("20000", "0"), "number of packets must be positive"),
    (SCATTERING.replace("20000", "-3"), "number of packets must be positive"),
    (SCATTERING.replace("seed: 7", "seed: 4294967296"),
     "random seed must fit 32 bits"),
    (SCATTERING.replace("seed: 7", "seed: -1"),
     "random seed must fit 32 bits"),
    (SCATTERING.replace("0.54", "1.5"), "dust albedo must be in [0, 1]"),
    (SCATTERING.replace("0.54", "-0.1"), "dust albedo must be in [0, 1]"),
    (SCATTERING.replace("0.44", "0."),
     "dust asymmetry must be non-zero and inside (-1, 1)"),
    (SCATTERING.replace("0.44", "1."),
     "dust asymmetry must be non-zero and inside (-1, 1)"),
    (SCATTERING.replace("0.44", "-1.5"),
     "dust asymmetry must be non-zero and inside (-1, 1)"),
] + [
    (_without(key), key + " is required for scattering off dust with a "
     "cross section above 0")
    for key in ("dust albedo", "dust asymmetry",
                "dust peak linear polarisation")
] + [
    (CHANNELS + "  scattered cubes: true\n",
     "scattered cubes needs scattering: true"),
    (SCATTERING + "  scattered cubes: true\n",
     "scattered cubes needs velocity channels"),
    ("  dust cross section per hydrogen: -1. m^2\n",
     "dust cross section per hydrogen must not be negative"),
]


@pytest.mark.parametrize("text, message", [
    (BLOCKS[block] + more, block + ":" + message)
    for block in sorted(BLOCKS) for more, message in SHARED_ERRORS
] + [
    (BLOCKS[block] + "  type: JPEG\n",
     "Unknown %s:type \"JPEG\" (BinaryArray or PGM)" % block)
    for block in sorted(BLOCKS)
] + [
    (IMAGES + "  number of views: 2\n  view phi 1: 0. degrees\n",
     "EmissionImages:view theta 1 is required"),
    (IMAGES + "  number of views: 2\n  view theta 1: 0. degrees\n",
     "EmissionImages:view phi 1 is required"),
    (IMAGES + "  number of views: 0\n",
     "EmissionImages:number of views must be 1..64"),
    (IMAGES + "  number of views: %d\n" % (MAX_VIEWS + 1),
     "EmissionImages:number of views must be 1..64"),
    (IMAGES + "  number of views: 2\n  view theta 1: 0. degrees\n"
     "  view phi 1: 0. degrees\n  sides x 1: -1. m\n",
     "the image sides must be positive"),
    (SKY + "  number of observers: 2\n",
     "EmissionSkyMaps:observer position 1 is required"),
    (SKY + "  number of observers: 0\n",
     "EmissionSkyMaps:number of observers must be 1..64"),
    (SKY + "  number of observers: %d\n" % (MAX_VIEWS + 1),
     "EmissionSkyMaps:number of observers must be 1..64"),
    (SKY + "  number of observers: 2\n"
     "  observer position 1: [0. m, 0. m, 0. m]\n"
     "  frame pole 1: [0., 0., 1.]\n  frame zero longitude 1: [0., 0., 2.]\n",
     "frame pole 1 and frame zero longitude 1 are parallel"),
    (SKY + "  number of observers: 2\n"
     "  observer position 1: [0. m, 0. m, 0. m]\n"
     "  exclusion radius 1: -1. m\n",
     "EmissionSkyMaps:exclusion radius 1 must be finite and not negative"),
])
def test_emission_driver_parameter_errors(tmp_path, text, message):
    text = "EmissivityValues:\n  Halpha: true\n" + \
        text.replace("EmissivityValues:\n  Halpha: true\n", "")
    r, used = _emission(tmp_path, text)
    assert r.returncode != 0 and message in r.stderr, r.stderr
    assert "Could not open" not in r.stderr
    assert not os.path.exists(used)


@pytest.mark.parametrize("block", sorted(BLOCKS))
def test_emission_driver_reads_the_scattering_keys_with_the_switch_only(
        tmp_path, block):
    """with `scattering: false` none of the keys of the scattered light is
    read, the switches included"""
    text = ("EmissivityValues:\n  Halpha: true\n" + BLOCKS[block] +
            SCATTERING.replace("scattering: true", "scattering: false") +
            "  scattered cubes: false\n")
    r, used = _emission(tmp_path, text, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    used = open(used).read()
    assert used.startswith(block + ":\n")
    keys = SCATTERING_KEYS + ("scattered cubes",)
    if block == "EmissionSkyMaps":
        keys += ("exclusion radius",)
    for key in keys:
        assert "  %s: value not used #" % key in used, (key, used)
    assert used.count("value not used") == len(keys)
    assert "  dust cross section per hydrogen: 2e-27 m^2 " in used


# ------------------------------------------------------- the library --

def test_library_exports_the_calls():
    import ctypes as C
    from cmacionize_amd import engine as E
    lib = E.load_library()
    assert E.MAX_VIEWS == MAX_VIEWS
    header = open(os.path.join(S.ROOT, "include", "cmi_gpu.h")).read()
    assert "#define CMI_GPU_MAX_VIEWS %d\n" % MAX_VIEWS in header
    for name in ("cmi_gpu_set_ccd_images", "cmi_gpu_set_sky_cameras",
                 "cmi_gpu_download_image_view",
                 "cmi_gpu_get_dust_view_counters",
                 "cmi_gpu_select_probe_view"):
        assert name in E.EXPORTED_SYMBOLS and hasattr(lib, name), name
    # null engines are refused before anything touches a device
    assert lib.cmi_gpu_set_ccd_images(None, 1, None, None, 8, 8, None,
                                      None) == S.EINVAL
    assert lib.cmi_gpu_set_sky_cameras(None, 1, None, None, 0., 1., 0., 1.,
                                       8, 4, None, 1) == S.EINVAL
    assert lib.cmi_gpu_download_image_view(None, 0, None, None, None) == \
        S.EINVAL
    assert lib.cmi_gpu_get_dust_view_counters(
        None, 0, (C.c_uint64 * 4)()) == S.EINVAL
    assert lib.cmi_gpu_select_probe_view(None, 0) == S.EINVAL
