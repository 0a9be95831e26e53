"""csrc/pt_workspace.h, the layout of a wavefront trace's workspace, on the host alone: tests/host/workspace_layout_check.cpp restates the size
formula, the three record-offset functions and the carving walk the header replaced, and compares them with it over a grid of tile counts,
samples, stage workgroups and record combinations -- every offset, every total, alignment, no overlap, everything inside the total.  Built
with the address and undefined-behaviour sanitizers.  A stand-alone program: nothing of it is loaded into Python.  CPU only."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_workspace_layout_equals_the_formulas_it_replaced_under_the_sanitizers():
    host = os.path.join(ROOT, "tests", "host")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "workspace_layout_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I" + os.path.join(ROOT, "gltf_renderer_amd", "csrc"), os.path.join(host, "workspace_layout_check.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
        assert "2800 cells, every offset and total as before" in r.stdout, r.stdout      # 10 x 5 x 7 x 8
