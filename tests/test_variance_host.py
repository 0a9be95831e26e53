"""The variance AOV and the noise report on the host (include/mipt.h pt_set_variance / pt_noise_estimate): the float32 restatement of
tests/variance_ref.py against float64, the struct layouts, and the calls that answer without a device."""
import ctypes as C

import numpy as np

from gltf_renderer_amd import abi, renderer
from tests import header_check as hc
from tests import variance_ref as vr

f32 = np.float32
PIXELS = 4096
COUNTS = (2, 3, 8, 64, 1024)
# The largest relative error of the float32 fold against the float64 population variance of the same float32 samples, per count, over
# PIXELS pixels x 4 channels of the samples below (seed 11), as measured on the CPU the test was written on.  The test allows 4 x these
# for other seeds, libraries and roundings of the samples' generation.  DESIGN.md section 4 has the same table.
MEASURED = {2: 6.5e-5, 3: 2.7e-6, 8: 3.8e-7, 64: 7.6e-7, 1024: 2.5e-6}


def heavy_tailed(rng, n, pixels):
    """n samples of `pixels` rgb pixels: log-normal radiance with a Pareto tail in a twentieth of the samples, 30 % of the samples exactly
    zero in all channels (paths that found no light)."""
    x = rng.lognormal(-1.0, 1.0, (n, pixels, 3))
    tail = rng.random((n, pixels, 1)) < 0.05
    x = np.where(tail, x * (1.0 + rng.pareto(1.5, (n, pixels, 1))) * 20.0, x)
    x = np.where(rng.random((n, pixels, 1)) < 0.30, 0.0, x)
    return x.astype(f32)


def population_variance64(x):
    """(pixels, 4) float64: per channel and of the channel sum, of the float32 samples x (n, pixels, 3)."""
    d = x.astype(np.float64)
    s = d.sum(axis=-1)
    return np.concatenate([d.var(axis=0), s.var(axis=0)[:, None]], axis=-1)


def test_the_float32_fold_against_the_float64_population_variance():
    rng = np.random.default_rng(11)
    for n in COUNTS:
        x = heavy_tailed(rng, n, PIXELS)
        assert float((x == 0).all(axis=-1).mean()) > 0.25
        _, targets = vr.fold(list(x))
        V = targets[-1]
        want = population_variance64(x)
        assert V.dtype == f32 and V.shape == (PIXELS, 4)
        assert np.all(V >= 0), n                                       # no entry is negative
        nz = want > 0
        assert np.all(V[~nz] == 0), n                                  # a pixel whose samples are all equal (all zero here): exactly 0
        rel = float((np.abs(V.astype(np.float64) - want)[nz] / want[nz]).max())
        print("n = %4d: largest relative error %.3e (recorded %.1e)" % (n, rel, MEASURED[n]))
        assert rel <= 4.0 * MEASURED[n], (n, rel)


def test_constant_samples_give_exactly_zero_and_one_sample_gives_zeros():
    rng = np.random.default_rng(12)
    c = heavy_tailed(rng, 1, 512)[0] + f32(0.37)
    _, targets = vr.fold([c] * 33)
    for k, V in enumerate(targets):
        assert np.all(V.view(np.uint32) == 0), k                       # +0 in every channel at every count
    _, one = vr.fold([heavy_tailed(rng, 1, 512)[0]])
    assert one[0].shape == (512, 4) and np.all(one[0].view(np.uint32) == 0)


def test_no_entry_is_negative_at_any_count():
    rng = np.random.default_rng(13)
    x = heavy_tailed(rng, 40, 2048)
    _, targets = vr.fold(list(x))
    for k, V in enumerate(targets):
        assert np.all(V >= 0) and np.all(np.isfinite(V)), k


def test_a_non_finite_product_leaves_the_variance_finite():
    big = f32(3e38)
    x = np.zeros((6, 4, 3), f32)
    x[1, 0] = (big, 0, 0)                  # d0 * d1 overflows in r, and in the channel sum
    x[2, 1] = (big, big, big)              # the channel sum itself overflows: s0 * s1 is inf * inf, or inf - inf on the way
    x[3, 2] = (np.inf, 0, 0)               # (never a sanitised sample; the select holds all the same)
    with np.errstate(all="ignore"):
        means, targets = vr.fold(list(x))
    for k, V in enumerate(targets):
        assert np.all(np.isfinite(V)), (k, V)
    assert np.all(targets[-1][3] == 0)     # the untouched pixel: constant zeros


def test_the_fold_continues_from_a_kept_mean_and_target():
    """What a batch, a resumed accumulation and an adaptive tile rely on: folding k samples onto (m, V) after n equals folding all n + k."""
    rng = np.random.default_rng(14)
    x = heavy_tailed(rng, 9, 256)
    means, targets = vr.fold(list(x))
    m2, t2 = vr.fold(list(x[4:]), first=4, m=means[3], V=targets[3])
    assert np.array_equal(t2[-1].view(np.uint32), targets[-1].view(np.uint32))
    assert np.array_equal(m2[-1].view(np.uint32), means[-1].view(np.uint32))


def test_the_noise_restatement_on_planted_values():
    W, H = 40, 24
    rng = np.random.default_rng(15)
    img = rng.random((H, W, 4)).astype(f32)
    var = (rng.random((H, W, 4)) * 0.1).astype(f32)
    var[3, 5, 3] = np.nan
    img[20, 33, :3] = -1.0                                             # a negative sum: the denominator is 1e-4
    ts = np.array([[4, 4, 0], [1, 4, 4]], np.uint32)
    mean, mx, px = vr.noise_tiles(img, var, ts)
    assert px.tolist() == [[256, 256, 128], [128, 128, 64]]
    assert mx[0, 0] == np.inf and mean[0, 0] == np.inf                 # the NaN counts as +infinity
    assert mean[0, 2] == -1 and mx[0, 2] == -1 and mean[1, 0] == -1 and mx[1, 0] == -1
    e = vr.pixel_error(img[20:21, 33:34], var[20:21, 33:34], 4)[0, 0]
    assert e == f32(np.sqrt(f32(var[20, 33, 3] / f32(3.0))) / f32(1e-4))
    tiles, est, above, smean, smax = vr.summary(mean.astype(f32), mx, px, ts, 0.5)
    assert (tiles, est) == (6, 4) and smax == np.inf and above >= 1


def test_struct_layouts_match_the_header():
    """The sizes the header's comments state (the layouts themselves: tests/test_host_abi.py)."""
    assert hc.stated_bytes("pt_variance_config") == C.sizeof(abi.PtVarianceConfig) == 16
    assert hc.stated_bytes("pt_noise_summary") == C.sizeof(abi.PtNoiseSummary) == 20


def test_calls_without_a_context_return_minus_one_and_write_nothing():
    """The argument check answers before anything touches a device: this test runs where there is none."""
    L = renderer.load_library()
    assert hasattr(L, "pt_set_variance") and hasattr(L, "pt_noise_estimate")
    cfg = abi.PtVarianceConfig(1, 0, 0x1000)
    assert L.pt_set_variance(None, C.byref(cfg)) == -1
    assert L.pt_set_variance(None, None) == -1
    mean, mx = np.full(6, 3.0, f32), np.full(6, 5.0, f32)
    s = abi.PtNoiseSummary(9, 9, 9, 9.0, 9.0)
    ts = np.full(6, 4, np.uint32)
    rc = L.pt_noise_estimate(None, C.c_void_p(0x1000), C.c_void_p(0x2000), 40, 24, ts.ctypes.data_as(C.c_void_p), 4, 0.1,
                             mean.ctypes.data_as(C.c_void_p), mx.ctypes.data_as(C.c_void_p), C.byref(s))
    assert rc == -1
    assert np.all(mean == 3.0) and np.all(mx == 5.0) and (s.tiles, s.tiles_estimated, s.tiles_above, s.mean, s.max) == (9, 9, 9, 9.0, 9.0)
