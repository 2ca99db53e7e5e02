"""Guard on the march loop of the emission-line images, from the compiler's
listing (`make asm`): every line_image_march_kernel<ND> is there, the loop
that holds its record loads has no scratch (spill) access, no atomic and no
call, and it loads the record in 16-B pieces - ND / 2 of them."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "cmacionize_amd", "csrc")
LISTING = os.path.join(CSRC, "engine.s")


@pytest.fixture(scope="module")
def loops():
    if not os.path.exists(LISTING):
        subprocess.run(["make", "-C", CSRC, "asm"], check=True)
    import line_image_loop
    with open(LISTING) as f:
        return line_image_loop.scan(f.read().split("\n"))


def test_every_record_size_has_its_kernel(loops):
    assert sorted(loops) == [2, 4, 6, 8], loops


def test_march_loop_has_no_scratch_no_atomic_no_call(loops):
    for nd, c in sorted(loops.items()):
        print(nd, c)
        assert c["scratch"] == 0, (nd, c)
        assert c["atomic"] == 0, (nd, c)
        assert c["calls"] == 0, (nd, c)
        assert c["loads"] == nd // 2, (nd, c)
        assert c["f64"] > 20, (nd, c)
