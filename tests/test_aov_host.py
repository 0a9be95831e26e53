"""CPU-only checks of the first-hit AOVs: the numpy restatement (tests/aov_ref.py) of the per-sample rules and the fold that
tests/test_gpu_aov.py holds the GPU to.  (The pt_aov_config mirror and the prototype of pt_set_aov: tests/test_host_abi.py.)"""
import ctypes as C
import os

import numpy as np

from gltf_renderer_amd import abi, renderer
from tests import adaptive_ref as ar
from tests import aov_ref as av

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = (0.25, 0.5, 0.75)


def test_the_library_exports_pt_set_aov_and_the_header_declares_it():
    """(The declaration against the binding: tests/test_host_abi.py.)"""
    L = renderer.load_library()
    assert "pt_set_aov" in renderer.EXPORTS and hasattr(L, "pt_set_aov")
    # no context: the argument check answers before anything touches a device
    cfg = abi.PtAovConfig(0, None, None)
    assert L.pt_set_aov(None, C.byref(cfg)) == -1


def frame(rows):
    return np.array(rows, f32).reshape(1, len(rows), -1)


def test_hit_mask_reads_hits_and_misses_exactly():
    hk = frame([[1, 0, 0, 1], [0, 1, 0, 1], list(ENV) + [1]])
    assert av.hit_mask(hk, ENV).tolist() == [[True, True, False]]
    bad = frame([[0.5, 0.5, 0.5, 1]])
    try:
        av.hit_mask(bad, ENV)
    except AssertionError:
        pass
    else:
        raise AssertionError("a pixel that is neither hit nor miss must be refused")


def test_a_miss_contributes_zeros_to_all_components():
    color = frame([[0.2, 0.4, 0.6, 1], list(ENV) + [1]])              # at a miss the COLOR frame shows the environment colour
    rec = av.albedo_record(color, np.array([[True, False]]))
    assert rec.tolist() == [[[f32(0.2), f32(0.4), f32(0.6), 1.0], [0.0, 0.0, 0.0, 0.0]]]


def test_a_non_finite_component_zeroes_the_whole_record_of_that_target():
    nan, inf = float("nan"), float("inf")
    rec = frame([[0.1, nan, 0.3, 1.0], [0.1, 0.2, inf, 1.0], [0.1, 0.2, 0.3, -inf], [0.1, 0.2, 0.3, 7.5]])
    out = av.sanitize(rec)
    assert out[0, :3].tolist() == [[0, 0, 0, 0]] * 3
    assert out[0, 3].tolist() == [f32(0.1), f32(0.2), f32(0.3), 7.5]
    assert av.albedo_record(frame([[nan, 0.5, 0.5, 1]]), np.array([[True]])).tolist() == [[[0, 0, 0, 0]]]   # coverage too


def test_blend4_is_blend_samples_weight_on_every_component():
    rng = np.random.default_rng(5)
    h, v = rng.random((3, 5, 4)).astype(f32), (10 * rng.random((3, 5, 4))).astype(f32)
    for n in (1, 2, 6, 255):
        b = f32(1.0) / f32(n + 1)
        want = h + b * (v - h)
        got = av.blend4(h, n, v)
        assert got.dtype == f32 and np.array_equal(got, want)
        assert np.array_equal(got[..., :3], ar.blend(h, n, v[..., :3])[..., :3])     # the beauty's own blend on rgb


def test_fold_blends_in_sample_order():
    rng = np.random.default_rng(6)
    recs = [rng.random((2, 2, 4)).astype(f32) for _ in range(9)]
    recs[3][0, 0] = 0                                                 # a miss among hits
    F = av.fold(recs)
    assert np.array_equal(F[0], recs[0])
    cur = recs[0]
    for n in range(1, 9):
        cur = cur + (f32(1.0) / f32(n + 1)) * (recs[n] - cur)
        assert np.array_equal(F[n], cur)
    assert np.allclose(F[8], np.mean(recs, axis=0), rtol=2e-6)
    # float32 blending does not commute: the order is part of the contract
    R = av.fold(recs[::-1])
    assert not np.array_equal(R[8], F[8])
    # coverage = the mean of the hit mask; rgb / coverage = the hit-only mean
    masks = [rng.random((4, 4)) < 0.6 for _ in range(8)]
    cols = [rng.random((4, 4, 4)).astype(f32) for _ in range(8)]
    A = av.fold([av.albedo_record(c, m) for c, m in zip(cols, masks)])[-1]
    cover = np.mean(masks, axis=0)
    assert np.allclose(A[..., 3], cover, atol=1e-6)
    hits = cover > 0
    want = np.sum([np.where(m[..., None], c[..., :3], 0) for c, m in zip(cols, masks)], axis=0)[hits] / np.sum(masks, axis=0)[hits][:, None]
    assert np.allclose(A[..., :3][hits] / A[..., 3][hits][:, None], want, rtol=1e-5)


def test_normal_encoding_round_trip_bound():
    """The bound of tests/test_gpu_aov.py: the encode rounds once, n + 1 <= 2 at up to 2^-24 (the halving is exact, the doubling of
    the decode gives that error back), and the decode rounds once, 2 c - 1 at up to 2^-25 (|2 c - 1| <= 1):
    |decode(encode(n)) - n| <= 2^-24 + 2^-25 < 2^-23."""
    rng = np.random.default_rng(7)
    n = rng.normal(size=(20000, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)
    n[:6] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    c = av.encode_normal(n)
    assert c.dtype == f32 and c.min() >= 0 and c.max() <= 1
    err = np.abs(av.decode_normal(c).astype(np.float64) - n.astype(np.float64))
    assert err.max() <= 2.0 ** -23
    assert np.array_equal(av.encode_normal(n), (n + f32(1)) / f32(2))


def test_render_gltf_aov_images():
    """tools/render_gltf.py --aov: albedo = rgb / coverage, normal = (n / |n| + 1) / 2 where coverage > 0, depth = the w channel."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("render_gltf", os.path.join(ROOT, "tools", "render_gltf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    alb = np.array([[[0.25, 0.5, 0.125, 0.5], [0, 0, 0, 0], [2.0, 0.0, 1.0, 1.0]]], f32)
    nd = np.array([[[0.0, 0.0, 0.5, 3.0], [0, 0, 0, 0], [0.0, 0.5, -0.5, 1.5]]], f32)      # means of normals: not unit length
    a8, n8, depth = mod.aov_images(alb, nd)
    assert a8.dtype == np.uint8 and a8.tolist() == [[[128, 255, 64], [0, 0, 0], [255, 0, 255]]]
    assert n8.tolist() == [[[128, 128, 255], [0, 0, 0], [128, 218, 37]]]
    assert depth.dtype == f32 and depth.tolist() == [[3.0, 0.0, 1.5]]
