"""csrc/pt_slab.h on the host alone: the node step's ray-space plane arithmetic (slab_axis / slab_near / slab_far), the candidate gate's
own-box arithmetic (own_box_t) and the builder's exact plane check, compiled by g++ into tests/host/slab_check.cpp -- the same inlines the
kernels compile, without contraction.  "The triangle's own box passes => every ancestor's node test passes", plane by plane, on more than
ten million planes: ray origins exactly on a plane, at the node origin (A = 0), inside, a hair off and far outside the node
(|A| >> 255 |S|), |inv| = 1 and 1e30 of either sign and everything between, q = 0 and 255, steps of 2^-20 and 2^13, and behind each plane
the bounds the builder may leave there (the nearest float on the admitted side first).  The same planes without the pad must land on the
wrong side, so the check cannot pass vacuously.  Then wide_write's byte search, restated over the same predicates: a bound with
fl(p + q s) == lo and p + q s > lo is turned down by the exact check and only by it.  A stand-alone program; CPU only."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_own_box_passing_implies_the_node_test_passing_on_ten_million_planes():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "slab_check")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I" + os.path.join(ROOT, "gltf_renderer_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "slab_check.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"with the pad: (\d+) planes, wrong side (\d+), dropped as NaN (\d+) \(in range (\d+)\)", r.stdout)
    planes, wrong, dropped, dropped_in_range = (int(x) for x in m.groups())
    assert planes >= 10_000_000 and wrong == 0
    assert dropped_in_range == 0 and dropped < 0.02 * planes          # a NaN only where (p - o) * inv or 255 * step * inv overflows
    m = re.search(r"without the pad: (\d+) planes, wrong side (\d+)", r.stdout)
    assert int(m.group(1)) == planes and int(m.group(2)) > 1000       # the pad is what makes it hold
    assert "worked lo example: float check alone 200, with the exact check 199, premise 1" in r.stdout
    assert "worked hi example: float check alone 200, with the exact check 201, premise 1" in r.stdout
    m = re.search(r"exact plane past the bound with the float check alone (\d+), with the exact check (\d+)", r.stdout)
    assert int(m.group(1)) > 0 and int(m.group(2)) == 0
