"""csrc/dev_buf.h, the owner of every device array of the context, on the host alone: tests/host/dev_buf_check.cpp drives DevBuf and TempBuf
over a counting stand-in for the five HIP calls they can make (tests/host/stub), built with the address and undefined-behaviour sanitizers.
A stand-alone program: nothing of it is loaded into Python.  CPU only."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dev_buf_frees_every_allocation_exactly_once_under_the_sanitizers():
    host = os.path.join(ROOT, "tests", "host")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "dev_buf_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I" + os.path.join(host, "stub"), "-I" + os.path.join(ROOT, "gltf_renderer_amd", "csrc"),
                               os.path.join(host, "dev_buf_check.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
        assert "4 allocations, 4 frees" in r.stdout and "nothing live" in r.stdout, r.stdout
