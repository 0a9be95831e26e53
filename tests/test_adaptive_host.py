"""CPU-only checks of tile-level adaptive sampling: the pt_adaptive_config mirror's layout, the C-ABI symbols, and the numpy restatement
of the per-tile error metric that tests/test_gpu_adaptive.py holds the GPU to."""
import ctypes as C
import math

import numpy as np

from gltf_renderer_amd import abi, renderer
from tests import adaptive_ref as ar

f32 = np.float32


def test_adaptive_config_layout():
    A = abi.PtAdaptiveConfig
    assert C.sizeof(A) == 16
    assert (A.enable.offset, A.min_samples.offset, A.max_samples.offset, A.threshold.offset) == (0, 4, 8, 12)
    assert "pt_set_adaptive" in renderer.EXPORTS and "pt_adaptive_read" in renderer.EXPORTS


def px(*rgb):
    return np.array([list(rgb) + [1.0]], f32)


def test_metric_zero_radiance_and_equal_images_give_zero():
    z = px(0, 0, 0)
    assert ar.pixel_error(z, z)[0] == 0.0
    c = px(0.6, 0.7, 0.9)
    assert ar.pixel_error(c, c)[0] == 0.0
    # zero radiance against a non-zero half buffer: the denominator is the 1e-4 floor
    e = ar.pixel_error(z, px(0.5, 0.25, 0.0))[0]
    assert e == f32(0.75) / f32(1e-4)


def test_metric_order_and_rounding_are_float32():
    I, A = px(1.0, 2.0, 3.0), px(0.5, 2.5, 2.0)
    d = (abs(f32(1.0) - f32(0.5)) + abs(f32(2.0) - f32(2.5))) + abs(f32(3.0) - f32(2.0))
    s = (f32(1.0) + f32(2.0)) + f32(3.0)
    want = d / (f32(1e-4) + np.sqrt(s))
    got = ar.pixel_error(I, A)[0]
    assert got.dtype == f32 and got == want
    assert abs(float(got) - 2.0 / (1e-4 + math.sqrt(6.0))) < 1e-6 * 2.0 / math.sqrt(6.0)


def test_metric_negative_channel_sum_clamps_the_square_root_to_zero():
    I, A = px(-3.0, 1.0, 0.5), px(-2.0, 1.0, 0.5)
    assert ar.pixel_error(I, A)[0] == f32(1.0) / f32(1e-4)


def test_metric_nan_counts_as_infinity():
    nan, inf = float("nan"), float("inf")
    assert ar.pixel_error(px(nan, 0, 0), px(0, 0, 0))[0] == np.inf
    assert ar.pixel_error(px(0, 0, 0), px(0, nan, 0))[0] == np.inf
    assert ar.pixel_error(px(inf, 0, 0), px(inf, 0, 0))[0] == np.inf          # inf - inf = NaN
    assert ar.pixel_error(px(inf, -inf, 0), px(0, 0, 0))[0] == np.inf         # NaN channel sum
    # a tile's error is the max, so one NaN pixel keeps the tile active whatever the threshold
    I = np.zeros((16, 16, 4), f32); A = I.copy()
    I[3, 5, 0] = nan
    assert ar.tile_errors(I, A)[0, 0] == np.inf


def test_tile_errors_ignore_pixels_outside_the_image_and_take_the_max():
    H, W = 20, 35                      # 2 x 3 tiles, ragged both ways
    rng = np.random.default_rng(1)
    I = rng.random((H, W, 4)).astype(f32)
    A = rng.random((H, W, 4)).astype(f32)
    E = ar.tile_errors(I, A)
    assert E.shape == (2, 3)
    e = ar.pixel_error(I, A)
    for ty in range(2):
        for tx in range(3):
            assert E[ty, tx] == e[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16].max()
    assert ar.tile_pixels(W, H).tolist() == [[256, 256, 48], [64, 64, 12]]


def test_fold_is_the_running_mean_and_the_half_buffer_takes_even_samples():
    rng = np.random.default_rng(2)
    raw = [np.concatenate([rng.random((4, 4, 3)).astype(f32), np.ones((4, 4, 1), f32)], axis=2) for _ in range(7)]
    I, A = ar.fold(raw)
    assert np.array_equal(I[0], raw[0]) and np.array_equal(A[0], raw[0]) and np.array_equal(A[1], raw[0])
    assert np.allclose(I[6][..., :3], np.mean([r[..., :3] for r in raw], axis=0), rtol=1e-5)
    assert np.allclose(A[6][..., :3], np.mean([raw[k][..., :3] for k in (0, 2, 4, 6)], axis=0), rtol=1e-5)
    assert np.array_equal(A[5], A[4])


def test_predict_retires_at_the_first_boundary_that_meets_the_rule():
    shape = (1, 3)
    # tile 0 converges at once, tile 1 at n = 6, tile 2 never
    table = {n: np.array([[0.0, 1.0 if n < 6 else 0.01, 5.0]], f32) for n in range(1, 17)}
    samples, err, calls = ar.predict(lambda n: table[n], 4, 3, 16, 0.05, shape)
    assert calls == [4, 8, 12, 16]
    assert samples.tolist() == [[4, 8, 16]]
    assert err[0, 0] == 0.0 and err[0, 1] == f32(0.01) and err[0, 2] == 5.0
    samples, _, calls = ar.predict(lambda n: table[n], 1, 3, 10, 0.05, shape)
    assert samples.tolist() == [[3, 6, 10]] and calls[-1] == 10
