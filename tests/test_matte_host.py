"""CPU-only checks of the ID mattes (include/mipt.h pt_set_matte, pt_matte_id, pt_matte_extract): pt_matte_id against a MurmurHash3_x86_32
written here, the exponent fix on integers, the constants against the header, the calls that answer without a device, and the restatement
(tests/matte_ref.py) that tests/test_gpu_matte.py holds the GPU to -- its own properties: a batch of S records equals S calls, the stated
order of the ranks, dropped ids, and the mask of pt_matte_extract.  (The pt_matte_config mirror and the prototypes: tests/test_host_abi.py.)"""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from gltf_renderer_amd import abi, renderer
from tests import header_check as hc
from tests import matte_ref as mr

f32, u32 = np.float32, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- MurmurHash3_x86_32, written from the algorithm's description (Appleby's reference: 4-byte little-endian blocks, a tail of up to three
# bytes, the length, the avalanche "fmix32"), independently of the library's and of tests/matte_ref.py's
def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & 0xffffffff


def murmur3_here(data, seed=0):
    h = seed
    nblocks = len(data) // 4
    for (k,) in struct.iter_unpack("<I", data[:4 * nblocks]):
        k = _rotl(k * 0xcc9e2d51 & 0xffffffff, 15) * 0x1b873593 & 0xffffffff
        h = (_rotl(h ^ k, 13) * 5 + 0xe6546b64) & 0xffffffff
    k = 0
    for i, byte in enumerate(data[4 * nblocks:]):
        k |= byte << (8 * i)
    if len(data) & 3:
        h ^= _rotl(k * 0xcc9e2d51 & 0xffffffff, 15) * 0x1b873593 & 0xffffffff
    h ^= len(data)
    for shift, mul in ((16, 0x85ebca6b), (13, 0xc2b2ae35)):
        h = ((h ^ (h >> shift)) * mul) & 0xffffffff
    return h ^ (h >> 16)


def fix_here(h):
    return h ^ (1 << 23) if ((h >> 23) & 0xff) in (0, 255) else h


def lib_id(data):
    return int(renderer.load_library().pt_matte_id(bytes(data), len(data)))


def test_matte_id_is_murmur3_with_the_exponent_fix():
    assert murmur3_here(b"hello") == 0x248bfa47 and (0x248bfa47 >> 23) & 0xff == 0x49          # the fix leaves it alone
    assert lib_id(b"hello") == 0x248bfa47 == mr.matte_id("hello") == renderer.Renderer.matte_id("hello")
    assert murmur3_here(b"") == 0 and lib_id(b"") == 1 << 23                                     # the empty name: raw hash 0, exponent 0
    rng = np.random.default_rng(11)
    for _ in range(400):
        data = rng.integers(0, 256, int(rng.integers(0, 41)), dtype=np.uint8).tobytes()
        want = fix_here(murmur3_here(data))
        assert lib_id(data) == want == mr.fix(mr.murmur3_32(data)), data
    for i in (0, 7, 95, 1000):
        for kind, stem in ((mr.INSTANCE, "instance_"), (mr.MATERIAL, "material_")):
            assert mr.default_id(kind, i) == lib_id((stem + str(i)).encode())


def test_the_fix_on_integers_and_on_names_whose_raw_hash_needs_it():
    for e in (0, 255):
        for rest in (0, 1, 0x7fffff, 0x80000000 | 0x123456):
            h = (rest & 0x807fffff) | (e << 23)
            g = mr.fix(h)
            assert g == h ^ (1 << 23) == fix_here(h) and (g >> 23) & 0xff in (1, 254)
    for h in (0x00800000, 0x3f800000, 0x7f000000, 0xff000000, 0x248bfa47):                        # exponents 1, 127, 254, 254, 0x49: unchanged
        assert mr.fix(h) == h
    # every fixed id reads as a finite, normal, non-zero float
    ids = np.array([mr.fix(h) for h in (0, 1, 0x7f800000, 0x7fc00000, 0xff800000, 0xffffffff, 0x80000000, 0x007fffff)], u32)
    v = ids.view(f32)
    assert np.all(np.isfinite(v)) and np.all(np.abs(v) >= np.finfo(f32).tiny) and np.all(ids != 0)
    # names whose raw hash has exponent 0 and 255, found by search: the library fixes them
    found = {0: None, 255: None}
    i = 0
    while None in found.values():
        name = b"object_%d" % i
        e = (murmur3_here(name) >> 23) & 0xff
        if e in found and found[e] is None:
            found[e] = name
        i += 1
        assert i < 200000
    for e, name in found.items():
        raw = murmur3_here(name)
        assert (raw >> 23) & 0xff == e and lib_id(name) == raw ^ (1 << 23) and (lib_id(name) >> 23) & 0xff == (1 if e == 0 else 254)


def test_the_matte_constants_are_the_headers():
    h = hc.header_text()
    assert (abi.MATTE_INSTANCE, abi.MATTE_MATERIAL, abi.MATTE_MAX_RANKS) == (0, 1, 8)
    assert re.search(r"enum\s*\{\s*PT_MATTE_INSTANCE\s*=\s*0\s*,\s*PT_MATTE_MATERIAL\s*=\s*1\s*\}", h)
    assert re.search(r"#define\s+PT_MATTE_MAX_RANKS\s+8\b", h)


def test_the_library_exports_the_matte_symbols_and_the_header_declares_them():
    """(The declarations against the binding: tests/test_host_abi.py.)"""
    L = renderer.load_library()
    for name in ("pt_set_matte", "pt_matte_id", "pt_matte_extract"):
        assert name in renderer.EXPORTS and hasattr(L, name), name
    h = hc.header_text()
    # the header says what a full pixel loses, and what must not be done to a layer
    assert "DROPPED" in h and "raises `ranks`" in h and "PT_EXCHANGE_REDUCE must not be used on a layer" in h


def test_calls_without_a_context_return_minus_one_and_write_nothing():
    """The argument check answers before anything touches a device: this test runs where there is none."""
    L = renderer.load_library()
    layer = np.full((4, 4, 4), 3.0, f32)
    cfg = abi.PtMatteConfig(1, 0, 2, 0)
    cfg.layers[0] = layer.ctypes.data
    assert L.pt_set_matte(None, C.byref(cfg), None) == -1
    assert L.pt_set_matte(None, None, None) == -1                       # a NULL config, likewise
    mask = np.full((4, 4), 5.0, f32)
    ptrs = (C.c_void_p * 1)(layer.ctypes.data)
    ids = np.array([1], u32)
    assert L.pt_matte_extract(None, ptrs, 2, 4, 4, ids.ctypes.data_as(C.c_void_p), 1, mask.ctypes.data_as(C.c_void_p)) == -1
    assert (mask == 5.0).all() and (layer == 3.0).all()


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def streams(rng, pixels, samples, n_ids, miss_share):
    """Random record streams (samples, pixels): ids drawn from n_ids names, a share of misses."""
    names = np.array([mr.default_id(mr.INSTANCE, i) for i in range(n_ids)], u32)
    rec = names[rng.integers(0, n_ids, (samples, pixels))]
    rec[rng.random((samples, pixels)) < miss_share] = 0
    return rec


def ordered(ids, cov):
    """The stated key on every adjacent pair of ranks."""
    a_id, b_id, a_c, b_c = ids[..., :-1].astype(np.int64), ids[..., 1:].astype(np.int64), cov[..., :-1], cov[..., 1:]
    a_ne, b_ne = a_id != 0, b_id != 0
    ok = (a_ne & ~b_ne) | ((a_ne == b_ne) & ((a_c > b_c) | ((a_c == b_c) & (a_id < b_id)))) | (~a_ne & ~b_ne)
    return bool(np.all(ok))


@pytest.mark.parametrize("K", [2, 4, 6, 8])
def test_a_batch_equals_the_calls_one_by_one_and_the_order_is_the_stated_one(K):
    rng = np.random.default_rng(K)
    P, S = 600, 16
    seen_more_than_k = seen_tie = 0
    for n_ids, miss in ((K + 3, 0.2), (K, 0.0), (3, 0.5), (2 * K + 4, 0.1)):
        rec = streams(rng, P, S, n_ids, miss)
        # equal-coverage ties: pixels that alternate between two ids end with two ranks of the same coverage
        a, b = mr.default_id(mr.INSTANCE, 0), mr.default_id(mr.INSTANCE, 1)
        rec[:, :40] = np.where((np.arange(S) % 2 == 0)[:, None], u32(a), u32(b))
        one = mr.fold(list(rec), K)                                        # S calls of one sample
        for split in ([S], [4, 4, 4, 4], [1, 5, 10], [9, 7]):
            ids, cov = mr.empty_state((P,), K)
            done = 0
            for s in split:
                ids, cov = mr.fold_call(ids, cov, list(rec[done:done + s]), done)
                done += s
                assert np.array_equal(ids, one[done - 1][0]) and np.array_equal(cov.view(u32), one[done - 1][1].view(u32)), (K, n_ids, split, done)
        ids, cov = one[-1]
        assert ordered(ids, cov)
        distinct = np.array([len(set(rec[:, p].tolist()) - {0}) for p in range(P)])
        seen_more_than_k += int((distinct > K).sum())
        for si, sc in one:                                                 # (after two samples the alternating pixels hold (a, 1/2), (b, 1/2))
            assert ordered(si, sc)
            ties = (si[:, :-1] != 0) & (si[:, 1:] != 0) & (sc[:, :-1] == sc[:, 1:])
            seen_tie += int(ties.any(axis=1).sum())
        # nothing dropped: the coverages sum to the hit fraction (here to rounding); dropped: strictly less
        hitfrac = (rec != 0).mean(axis=0)
        total = cov.astype(np.float64).sum(axis=1)
        full = distinct <= K
        assert np.all(np.abs(total[full] - hitfrac[full]) < 1e-5)
        assert np.all(total[~full] < hitfrac[~full] - 1e-3)
        # every id a pixel holds is one it saw, no id twice
        for p in range(0, P, 37):
            held = [i for i in ids[p].tolist() if i]
            assert len(held) == len(set(held)) and set(held) <= set(rec[:, p].tolist())
    assert seen_more_than_k >= 50 and seen_tie >= 40, (seen_more_than_k, seen_tie)


def test_a_call_that_does_not_accumulate_keeps_the_last_sample():
    rng = np.random.default_rng(5)
    rec = streams(rng, 200, 5, 6, 0.3)
    ids, cov = mr.empty_state((200,), 4)
    ids[:] = 77; cov[:] = 0.25                                             # whatever was there
    ids, cov = mr.fold_call(ids, cov, list(rec), -1)
    last = rec[-1]
    assert np.array_equal(ids[:, 0], last) and np.array_equal(cov[:, 0], (last != 0).astype(f32))
    assert np.all(ids[:, 1:] == 0) and np.all(cov[:, 1:].view(u32) == 0)


def test_the_sort_is_a_function_of_the_multiset():
    rng = np.random.default_rng(9)
    ids = np.array([[5, 0, 9, 3, 0, 7]], u32)
    cov = np.array([[0.25, 0, 0.5, 0.25, 0, 0.125]], f32)
    want_ids, want_cov = np.array([[9, 3, 5, 7, 0, 0]], u32), np.array([[0.5, 0.25, 0.25, 0.125, 0, 0]], f32)
    for _ in range(50):
        p = rng.permutation(6)
        a, b = mr.sort_ranks(ids[:, p], cov[:, p])
        assert np.array_equal(a, want_ids) and np.array_equal(b, want_cov)
    # unsigned order: an id with the top bit set comes after a small one at equal coverage
    a, _ = mr.sort_ranks(np.array([[0x80000001, 2]], u32), np.array([[0.5, 0.5]], f32))
    assert a.tolist() == [[2, 0x80000001]]


def test_pack_and_unpack_are_cryptomattes_rgba_layout():
    ids = np.arange(1, 1 + 2 * 3 * 6, dtype=u32).reshape(2, 3, 6) * u32(0x01010101)
    cov = (np.arange(2 * 3 * 6, dtype=f32).reshape(2, 3, 6) / f32(64)).astype(f32)
    layers = mr.pack(ids, cov)
    assert len(layers) == 3 and layers[0].shape == (2, 3, 4) and layers[0].dtype == f32
    for j, l in enumerate(layers):
        assert np.array_equal(l.view(u32)[..., 0], ids[..., 2 * j]) and np.array_equal(l[..., 1], cov[..., 2 * j])
        assert np.array_equal(l.view(u32)[..., 2], ids[..., 2 * j + 1]) and np.array_equal(l[..., 3], cov[..., 2 * j + 1])
    i2, c2 = mr.unpack(layers)
    assert np.array_equal(i2, ids) and np.array_equal(c2, cov)


def test_extract_sums_the_ranks_in_order():
    B = 0x40000000                                                         # ids with a normal exponent: the fix leaves them alone
    ids = np.array([[B + 9, B + 3, B + 5, B + 7], [B + 3, 0, 0, 0], [0, 0, 0, 0]], u32)
    cov = np.array([[0.5, 0.25, 0.125, 0.0625], [1, 0, 0, 0], [0, 0, 0, 0]], f32)
    assert mr.extract(ids, cov, [B + 3, B + 7]).tolist() == [0.3125, 1.0, 0.0]
    assert mr.extract(ids, cov, [B + 11]).tolist() == [0.0, 0.0, 0.0]
    # the set goes through the fix: 0 stands for fix(0), which no empty rank equals
    assert mr.extract(ids, cov, [0]).tolist() == [0.0, 0.0, 0.0]
    # sequential float32: ((a + b) + c), not a + (b + c)
    c = np.array([[1.0, 2.0 ** -24, 2.0 ** -24]], f32)
    assert mr.extract(np.array([[B + 1, B + 2, B + 3]], u32), c, [B + 1, B + 2, B + 3])[0] == f32(1.0)


def test_render_gltf_writes_a_layer_as_a_32_bit_float_rgba_exr_bit_for_bit(tmp_path):
    """tools/render_gltf.py --matte-out: the ids are bit patterns, so the file must hold every channel's 32 bits."""
    import importlib.util
    import struct as st
    from gltf_renderer_amd import gltf
    spec = importlib.util.spec_from_file_location("render_gltf", os.path.join(ROOT, "tools", "render_gltf.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(3)
    Hh, Ww = 5, 7
    ids = np.array([mr.default_id(mr.INSTANCE, int(i)) for i in rng.integers(0, 50, Hh * Ww * 2)], u32).reshape(Hh, Ww, 2)
    layer = np.zeros((Hh, Ww, 4), f32)
    layer.view(u32)[..., 0::2] = ids
    layer[..., 1::2] = rng.random((Hh, Ww, 2)).astype(f32)
    path = str(tmp_path / "layer_00.exr")
    tool.write_exr_rgba32f(path, layer)
    rgb, half = gltf.load_rgb32f(path)                                    # the library's own EXR reader: R, G, B
    assert not half and np.array_equal(rgb.view(u32), layer[..., :3].view(u32))
    raw = open(path, "rb").read()                                         # A: the first channel of every scanline (alphabetical order)
    line = 8 + 16 * Ww
    body = raw[len(raw) - Hh * line:]
    for y in range(Hh):
        assert st.unpack_from("<ii", body, y * line) == (y, 16 * Ww)
        assert np.array_equal(np.frombuffer(body, u32, Ww, y * line + 8), layer[y, :, 3].view(u32))
