"""CPU-only checks of the accumulation checkpoint (include/mipt.h pt_accum_save / pt_accum_load / pt_accum_inspect): the section flags
against the header, pt_accum_inspect on blobs written by the independent writer tests/checkpoint_ref.py -- every field read
back, every refusal the header promises, one malformation a case -- and a sanitizer-instrumented mutation fuzzer of the validator
(tests/fuzz/accum_fuzz.cpp), a stand-alone program built from accum_state.cpp alone."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from gltf_renderer_amd import abi, renderer
from tests import checkpoint_ref as cr
from tests import header_check as hc

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def inspect(blob):
    L = renderer.load_library()
    info = abi.PtAccumInfo()
    rc = L.pt_accum_inspect(bytes(blob), len(blob), C.byref(info))
    return rc, info


def image(rng, w, h):
    return rng.standard_normal((h, w, 4)).astype(f32)


def blob_uniform(w=72, h=40, frames=7, **kw):
    rng = np.random.default_rng(11)
    return cr.write(w, h, frames, image(rng, w, h), world_to_clip=rng.standard_normal(16), **kw)


def blob_full(w=72, h=40, rank=1, world=3, frames=6, config=(1, 2, 16, 0.125), next_frame=6):
    """All four sections: active tiles hold `frames` samples, retired ones fewer."""
    rng = np.random.default_rng(12)
    n = len(cr.rank_tiles(w, h, rank, world))
    active = (np.arange(n) % 2).astype(np.uint32)
    samples = np.where(active == 1, frames, np.maximum(frames - 2 - np.arange(n) % 3, 0)).astype(np.uint32)
    error = rng.random(n).astype(f32)
    if n:
        error[0] = np.inf                                            # a NaN pixel counts as +inf: a legal error
    ad = dict(config=config, active=active, samples=samples, error=error, half=image(rng, w, h))
    return cr.write(w, h, frames, image(rng, w, h), image(rng, w, h), image(rng, w, h), ad, rank, world, next_frame, rng.standard_normal(16))


def patched(blob, offset, fmt, value, reseal=True):
    b = bytearray(blob)
    b[offset:offset + struct.calcsize(fmt)] = struct.pack(fmt, value)
    return cr.seal(b) if reseal else bytes(b)


def test_mirrors_match_the_header_and_the_library_exports_the_three_calls():
    """The section flags and the exports (the pt_accum_images / pt_accum_info mirrors and the three prototypes: tests/test_host_abi.py)."""
    assert (abi.ACCUM_OUTPUT, abi.ACCUM_ALBEDO, abi.ACCUM_NORMAL_DEPTH, abi.ACCUM_ADAPTIVE) == (1, 2, 4, 8)
    assert "PT_ACCUM_OUTPUT = 1 << 0, PT_ACCUM_ALBEDO = 1 << 1, PT_ACCUM_NORMAL_DEPTH = 1 << 2, PT_ACCUM_ADAPTIVE = 1 << 3" in hc.header_text(comments=False)
    L = renderer.load_library()
    for name in ("pt_accum_save", "pt_accum_load", "pt_accum_inspect"):
        assert name in renderer.EXPORTS and hasattr(L, name), name
    # no context, no blob: answered before anything touches a device
    n = C.c_size_t()
    assert L.pt_accum_save(None, None, 4, 4, 0, 1, 0, None, 0, C.byref(n)) == INVALID
    assert L.pt_accum_load(None, None, 0, None) == INVALID
    assert L.pt_accum_inspect(None, 0, None) == INVALID


def test_the_header_comment_gives_the_offsets_the_writer_uses():
    """The field table of include/mipt.h, read as (offset, type) pairs, is the layout tests/checkpoint_ref.py packs."""
    m = re.search(r"Header, 160 bytes:(.*?)Payload, from offset 160", hc.header_text(), re.S)
    assert m
    rows = re.findall(r"^\s*\*\s+(?:offset\s+)?(\d+)\s+(char\[8\]|u32\[4\]|f32\[16\]|u32|u64|i32|pt_adaptive_config)", m.group(1), re.M)
    size = {"char[8]": 8, "u32": 4, "u64": 8, "i32": 4, "f32[16]": 64, "pt_adaptive_config": 16, "u32[4]": 16}
    at = 0
    for off, typ in rows:
        assert int(off) == at, (off, typ)
        at += size[typ]
    assert at == 160 and len(rows) == 16
    code = {"char[8]": "8s", "u32": "I", "u64": "Q", "i32": "i", "f32[16]": "16f", "pt_adaptive_config": "3if", "u32[4]": "4I"}
    assert "<" + "".join(code[t] for _, t in rows) == cr.HEADER


CASES = {
    "uniform_72x40": lambda: (blob_uniform(), dict(sections=1, width=72, height=40, tile_rank=0, tile_rank_count=1, accumulated_frames=7, tiles=15,
                                                   next_frame=0, adaptive=(0, 0, 0, 0.0))),
    "all_sections_rank_1_of_3": lambda: (blob_full(), dict(sections=15, width=72, height=40, tile_rank=1, tile_rank_count=3, accumulated_frames=6, tiles=5,
                                                           next_frame=6, adaptive=(1, 2, 16, 0.125))),
    "1x1": lambda: (blob_full(1, 1, 0, 1, 3, (1, 2, 2, 0.0), 2 ** 40 + 3), dict(sections=15, width=1, height=1, tile_rank=0, tile_rank_count=1,
                                                                             accumulated_frames=3, tiles=1, next_frame=2 ** 40 + 3, adaptive=(1, 2, 2, 0.0))),
    "17x16_ragged_column": lambda: (blob_uniform(17, 16, 1, albedo=np.ones((16, 17, 4), f32), next_frame=9),
                                    dict(sections=3, width=17, height=16, tile_rank=0, tile_rank_count=1, accumulated_frames=1, tiles=2, next_frame=9,
                                         adaptive=(0, 0, 0, 0.0))),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_inspect_accepts_the_reference_writers_blobs_and_reads_every_field_back(name):
    blob, want = CASES[name]()
    rc, info = inspect(blob)
    assert rc == 0
    got = {k: getattr(info, k) for k in want if k != "adaptive"}
    a = info.adaptive
    got["adaptive"] = (a.enable, a.min_samples, a.max_samples, a.threshold)
    assert got == want
    assert info.total_bytes == len(blob)
    images = bin(want["sections"] & 7).count("1")
    P = cr.packed_bytes(want["width"], want["height"], want["tile_rank"], want["tile_rank_count"])
    assert P == want["tiles"] * 4096 == renderer.load_library().pt_tiles_packed_bytes(want["width"], want["height"], want["tile_rank"], want["tile_rank_count"])
    assert len(blob) == 160 + images * P + ((want["tiles"] * 16 + P) if want["sections"] & 8 else 0)
    d = cr.parse(blob)                                                # the parser agrees with its own writer
    assert d["accumulated_frames"] == want["accumulated_frames"] and d["sections"] == want["sections"]


def test_a_rank_beyond_the_tile_grid_owns_nothing_and_is_a_legal_blob():
    blob = cr.write(16, 16, 2, np.ones((16, 16, 4), f32), rank=2, world=3)
    assert len(blob) == 160
    rc, info = inspect(blob)
    assert rc == 0 and info.tiles == 0 and info.total_bytes == 160


def test_every_truncation_is_refused():
    for blob in (blob_uniform(), blob_full()):
        for n in range(160):
            assert inspect(blob[:n])[0] == INVALID, n
        assert inspect(blob[:-1])[0] == INVALID
        assert inspect(blob + b"\0")[0] == INVALID
        # ... also when total_bytes and the crc are made to agree with the new length: the section sizes do not
        for cut in (blob[:-1], blob + b"\0"):
            assert inspect(patched(cut, 16, "<Q", len(cut)))[0] == INVALID


FIELD_FLIPS = [
    ("magic", 0, "<8s", b"MIPTACC2"), ("version", 8, "<I", 2), ("header_bytes", 12, "<I", 164), ("total_bytes", 16, "<Q", 1 << 40),
    ("sections_without_albedo", 28, "<I", 13), ("width_zero", 32, "<I", 0), ("width_other_grid", 32, "<I", 96), ("height_zero", 36, "<I", 0),
    ("height_other_grid", 36, "<I", 56), ("tile_rank_equals_count", 40, "<I", 3), ("tile_rank_beyond_count", 40, "<I", 0xffffffff), ("tile_rank_count_zero", 44, "<I", 0),
    ("tile_rank_count_other_share", 44, "<I", 2), ("accumulated_frames_zero", 48, "<i", 0), ("accumulated_frames_negative", 48, "<i", -6),
    ("accumulated_frames_below_a_tile", 48, "<i", 5), ("tiles", 52, "<I", 6), ("adaptive_enable_zero", 128, "<i", 0), ("adaptive_max_below_min", 136, "<i", 1),
    ("adaptive_threshold_negative", 140, "<f", -0.5), ("adaptive_threshold_inf", 140, "<f", float("inf")),
    ("reserved_0", 144, "<I", 1), ("reserved_3", 156, "<I", 0x80000000),
]


@pytest.mark.parametrize("case", FIELD_FLIPS, ids=[c[0] for c in FIELD_FLIPS])
def test_a_flipped_header_field_is_refused_by_its_own_check(case):
    """The crc is recomputed after the flip, so it is the field's check that fires; the untouched blob passes."""
    _, offset, fmt, value = case
    blob = blob_full()
    assert inspect(blob)[0] == 0
    assert inspect(patched(blob, offset, fmt, value))[0] == INVALID
    assert inspect(patched(blob, offset, fmt, value, reseal=False))[0] == INVALID


def test_fields_that_carry_no_check_may_change_under_a_fresh_crc():
    """next_frame and the camera are the caller's data: any value is legal -- which shows that resealing works, so that the refusals above
    are the field checks' and not the crc's."""
    blob = blob_full()
    rc, info = inspect(patched(blob, 56, "<Q", 2 ** 63 + 5))
    assert rc == 0 and info.next_frame == 2 ** 63 + 5
    assert inspect(patched(blob, 64, "<f", float("nan")))[0] == 0
    assert inspect(patched(blob, 56, "<Q", 77, reseal=False))[0] == INVALID          # without the new crc: refused


def test_a_flipped_payload_byte_fails_the_crc():
    for blob in (blob_uniform(), blob_full()):
        for at in (160, 160 + 4096 + 5, len(blob) - 1):
            b = bytearray(blob)
            b[at] ^= 0x10
            assert inspect(b)[0] == INVALID, at
        b = bytearray(blob)
        b[24] ^= 1                                                    # ... and so does a flipped crc
        assert inspect(b)[0] == INVALID


def test_a_width_above_two_to_the_thirty_is_refused_in_64_bit_arithmetic():
    """width 2^30 + 1, with tiles, total_bytes and the crc all consistent with it: a 160-byte blob of a rank that owns no tile."""
    w = 2 ** 30 + 1
    tiles_x = (w + 15) // 16
    head = struct.pack(cr.HEADER, cr.MAGIC, 1, 160, 160, 0, 1, w, 1, tiles_x, tiles_x + 1, 1, 0, 0, *([0.0] * 16), 0, 0, 0, 0.0, 0, 0, 0, 0)
    assert inspect(cr.seal(head))[0] == INVALID
    ok = struct.pack(cr.HEADER, cr.MAGIC, 1, 160, 160, 0, 1, 2 ** 30, 1, tiles_x, tiles_x + 1, 1, 0, 0, *([0.0] * 16), 0, 0, 0, 0.0, 0, 0, 0, 0)
    rc, info = inspect(cr.seal(ok))                                   # 2^30 itself is legal: the bound, not the shape, refused the other
    assert rc == 0 and info.width == 2 ** 30 and info.tiles == 0
    # a tile count whose byte size overflows 32 bits is computed in 64: 2^30 x 2^30 has 2^52 tiles, of which rank 0 of 2^31 owns 2^21
    big = struct.pack(cr.HEADER, cr.MAGIC, 1, 160, 160, 0, 1, 2 ** 30, 2 ** 30, 0, 2 ** 31, 1, 2 ** 21, 0, *([0.0] * 16), 0, 0, 0, 0.0, 0, 0, 0, 0)
    assert inspect(cr.seal(big))[0] == INVALID                        # total_bytes would be 160 + 2^33


def test_tiles_off_by_one_is_refused():
    blob = blob_uniform()
    for t in (14, 16):
        assert inspect(patched(blob, 52, "<I", t))[0] == INVALID
        # ... also with a payload of exactly that many tiles
        grown = patched(blob[:160] + bytes(t * 4096), 52, "<I", t, reseal=False)
        assert inspect(patched(grown, 16, "<Q", len(grown)))[0] == INVALID


def test_an_adaptive_config_pt_set_adaptive_refuses_is_refused():
    assert inspect(blob_full(config=(1, 1, 16, 0.125)))[0] == INVALID             # min_samples 1
    assert inspect(blob_full(config=(1, 2, 16, float("nan"))))[0] == INVALID      # a NaN threshold
    assert inspect(blob_full(config=(1, 2, 16, 0.0)))[0] == 0
    # without the section the config bytes are zero
    blob = blob_uniform()
    assert inspect(patched(blob, 132, "<i", 2))[0] == INVALID
    assert inspect(patched(blob, 140, "<f", 0.5))[0] == INVALID


def test_bad_tile_records_are_refused():
    blob = blob_full()
    d = cr.parse(blob)
    rec0 = 160 + 3 * d["tiles"] * 4096
    assert d["records"][1, 0] == 1 and d["records"][0, 0] == 0       # tile 1 is active, tile 0 retired
    assert inspect(patched(blob, rec0 + 16 + 4, "<I", 5))[0] == INVALID           # an active tile with a short count
    assert inspect(patched(blob, rec0 + 4, "<I", 7))[0] == INVALID                # a retired tile beyond accumulated_frames
    assert inspect(patched(blob, rec0, "<I", 2))[0] == INVALID                    # active > 1
    assert inspect(patched(blob, rec0 + 8, "<f", float("nan")))[0] == INVALID     # a NaN error
    assert inspect(patched(blob, rec0 + 12, "<I", 1))[0] == INVALID               # a non-zero pad
    assert inspect(patched(blob, rec0 + 4, "<I", 6))[0] == 0                      # a retired tile at the full count is legal


def test_unknown_section_bits_and_a_missing_output_are_refused():
    blob = blob_uniform()
    assert inspect(patched(blob, 28, "<I", 1 | 16))[0] == INVALID                 # bit 4
    assert inspect(patched(blob, 28, "<I", 1 | 0x80000000))[0] == INVALID
    assert inspect(patched(blob, 28, "<I", 2))[0] == INVALID                      # one image, but it is not the output
    assert inspect(patched(blob_full(), 28, "<I", 14))[0] == INVALID
    assert inspect(patched(blob, 28, "<I", 0))[0] == INVALID


def write_seeds(d):
    seeds = {"uniform": blob_uniform(), "full": blob_full(), "one": blob_full(1, 1, 0, 1, 3, (1, 2, 2, 0.0)), "ragged": blob_uniform(17, 16, 1),
             "empty_rank": cr.write(16, 16, 2, np.ones((16, 16, 4), f32), rank=2, world=3)}
    for name, blob in seeds.items():
        open(os.path.join(d, name + ".acc"), "wb").write(blob)


def test_the_validator_survives_mutated_blobs_under_the_sanitizers():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = [os.path.join(ROOT, p) for p in ("tests/fuzz/accum_fuzz.cpp", "gltf_renderer_amd/csrc/host/accum_state.cpp")]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, ".accum_fuzz")
        flags = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        probe = os.path.join(d, "probe.cpp")
        open(probe, "w").write("int main() { return 0; }\n")
        if subprocess.run(flags + [probe, "-o", os.path.join(d, ".probe")], capture_output=True).returncode != 0:
            pytest.skip("g++ cannot link the sanitizer runtimes here")
        subprocess.check_call(flags + ["-I" + os.path.join(ROOT, "include")] + src + ["-o", exe])      # the fuzzer itself must compile
        write_seeds(d)
        for args in (("6000", "201"), ("6000", "202")):
            r = subprocess.run([exe, d] + list(args), capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
            m = re.search(r"fuzz: (\d+) iterations over 5 seeds, (\d+) accepted, (\d+) refused", r.stdout)
            assert m, r.stdout
            assert int(m.group(2)) > 50 and int(m.group(3)) > 1000, r.stdout   # both sides of the validator were reached


def test_the_render_tool_refuses_a_checkpoint_that_does_not_fit_its_command_line():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render_gltf
    flags = (abi.ACCUM_ALBEDO, abi.ACCUM_NORMAL_DEPTH, abi.ACCUM_ADAPTIVE)
    _, full = inspect(blob_full(rank=0, world=1))                    # 72x40, AOVs, adaptive (2, 16, 0.125)
    _, plain = inspect(blob_uniform())
    fit = render_gltf.resume_mismatch
    assert fit(full, (72, 40), True, (2, 16, 0.125), flags) is None
    assert fit(plain, (72, 40), False, None, flags) is None
    assert "--size" in fit(full, (72, 41), True, (2, 16, 0.125), flags)
    assert "--aov" in fit(full, (72, 40), False, (2, 16, 0.125), flags) and "--aov" in fit(plain, (72, 40), True, None, flags)
    assert "--adaptive" in fit(full, (72, 40), True, None, flags) and "--adaptive" in fit(plain, (72, 40), False, (2, 16, 0.125), flags)
    for cfg in ((3, 16, 0.125), (2, 32, 0.125), (2, 16, 0.25)):
        assert "--min-spp" in fit(full, (72, 40), True, cfg, flags)
    _, shard = inspect(blob_full())
    assert "shard" in fit(shard, (72, 40), True, (2, 16, 0.125), flags)
