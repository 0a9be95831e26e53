"""One thread per scene on the plain-C++ scene side (tests/host/threads_check.cpp): eight threads whose FIRST call into the image
decoders, the PNG writer, the glTF / GLB loader and the checkpoint validator is concurrent, each compared byte for byte with a serial
repeat.  CPU only; the program is a stand-alone executable built twice, with -fsanitize=thread and plain -O2, and every phase runs in a
process of its own so that each lazily built table is built under contention.  The sanitized png and gltf-datauri phases are the ones
that reported races on the inflate / crc / base64 tables before those became statics initialised in their declaration.

Like every race test these detect races, they do not prove their absence: the plain build only shows a race that happened to corrupt
a result in that run, the sanitized build only the accesses that run executed."""
import os, shutil, struct, subprocess, sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PHASES = ("png", "images", "gltf-datauri", "glb", "errors", "accum")
SOURCES = ("tests/host/threads_check.cpp", "gltf_renderer_amd/csrc/host/image_decode.cpp", "gltf_renderer_amd/csrc/host/gltf_scene.cpp",
           "gltf_renderer_amd/csrc/host/accum_state.cpp")
FLAGS = {"tsan": ["-fsanitize=thread", "-O1", "-g"], "plain": ["-O2"]}


def build(exe, flags, sources=SOURCES):
    subprocess.check_call(["g++", "-std=c++17", "-pthread"] + flags + ["-I" + os.path.join(ROOT, "include")] + [os.path.join(ROOT, p) for p in sources] + ["-o", exe])


def first_deflate_block_type(png):
    """BTYPE of the first deflate block of a PNG's first IDAT chunk (RFC 1951 3.2.3: 1 = fixed, 2 = dynamic Huffman codes)."""
    at = 8
    while at < len(png):
        n, kind = struct.unpack(">I4s", png[at:at + 8])
        if kind == b"IDAT":
            return (png[at + 8 + 2] >> 1) & 3           # behind the two bytes of the zlib header
        at += 12 + n
    raise AssertionError("no IDAT chunk")


@pytest.fixture(scope="module")
def seeds(tmp_path_factory):
    """The seed files of tools/fuzz_host.py, the two scene containers with a camera added, and a dynamic-Huffman PNG."""
    import fuzz_host
    import test_gltf_loader as tl
    d = str(tmp_path_factory.mktemp("threads_seeds"))
    fuzz_host.write_seeds(d)
    for embed, name in (("view", "sink.glb"), ("uri", "sink.gltf")):
        b = tl.build_kitchen_sink(embed)
        b.j["cameras"] = [{"type": "perspective", "perspective": {"aspectRatio": 1.5, "yfov": 0.8, "znear": 0.05, "zfar": 250.0}},
                          {"type": "orthographic", "orthographic": {"xmag": 2.0, "ymag": 0.5, "znear": 0.01, "zfar": 40.0}}]
        b.node(root=True, name="camera", camera=1, translation=[0, 1, 5])
        (b.write_glb if embed == "view" else b.write_gltf)(os.path.join(d, name))
    text = open(os.path.join(d, "sink.gltf")).read()
    assert text.count('"uri": "data:') == 13      # the buffer and the twelve images: base64
    png = tl.png_bytes(tl.smooth_image(np.random.default_rng(11), 45, 61, 4))
    assert first_deflate_block_type(png) == 2, "the PNG written for the dynamic-Huffman path does not start with a dynamic block"
    open(os.path.join(d, "dynamic.png"), "wb").write(png)
    return d


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = str(tmp_path_factory.mktemp("threads_check"))
    exes = {"plain": os.path.join(d, "threads_check")}
    build(exes["plain"], FLAGS["plain"])
    try:
        exes["tsan"] = os.path.join(d, "threads_check_tsan")
        build(exes["tsan"], FLAGS["tsan"])
    except subprocess.CalledProcessError:
        exes["tsan"] = None
    return exes


@pytest.mark.parametrize("phase", PHASES)
@pytest.mark.parametrize("kind", ["tsan", "plain"])
def test_eight_threads_first_use_equals_the_serial_repeat(programs, seeds, kind, phase, tmp_path):
    exe = programs[kind]
    if exe is None:
        pytest.skip("g++ cannot link the thread sanitizer's runtime here")
    work = str(tmp_path / "work")                       # a copy per run: the phases write there
    shutil.copytree(seeds, work)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, phase, work], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-500:])
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "ThreadSanitizer" not in r.stderr and "WARNING" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith(phase + ": 8 threads") and "all equal" in r.stdout
