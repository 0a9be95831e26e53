"""The environments and configs that tests/test_envfilter_host.py (E32 on the CPU) and tests/test_gpu_envfilter.py (the kernels) both use: the
smallest shapes at which pt_env_filter's kernels can still go wrong.

  a  N = 9   a random 64 x 32 equirect; ggx_mips 3 -> levels 9, 4, 2 at a = 0, 0.25, 1; 16 and 256 GGX samples; diffuse resolution 8
  b  N = 2   an 8 x 4 equirect: cube mips 2 and 1, every tap of the 1 x 1 mip re-projects; ggx_mips 2; diffuse resolution 1 and 3
  c  N = 33  scenes.sky_image(256, 128) with the all-default config: odd size, the reference's mip rule -> 2 levels, a 256^2 diffuse cube
             (every GGX texel, a fixed random subset of 2000 diffuse texels)
  d  N = 5   a crafted raw cube (the test hook's way in) with one very bright texel at a face corner
"""
import numpy as np

from gltf_renderer_amd import abi, scenes
from tests import envfilter_ref as er

f16, f32 = np.float16, np.float32


def config(**kw):
    return abi.PtEnvFilterConfig(**dict(er.DEFAULTS, **kw))


def random_equirect(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w, 3)) ** 3 * 6).astype(f32)


def bright_corner_cube():
    """N = 5: values around 1, and 6e4 (near the largest half) in texel (0, 0) of face 0, whose three neighbours across the corner are
    reached only by re-projection."""
    rng = np.random.default_rng(5)
    cube = np.zeros((6, 5, 5, 4), f16)
    cube[..., :3] = (rng.random((6, 5, 5, 3)) * 2).astype(f16)
    cube[0, 0, 0, :3] = (6.0e4, 3.0e4, 1.0e4)
    cube[..., 3] = 1
    return cube.view(np.uint16)


def unit_pyramid():
    """A valid importance pyramid for pt_debug_env_create_raw (the filter never reads it): ones, and their 2 x 2 sums up to the apex."""
    return np.concatenate([np.full((1024 >> l) ** 2, 4.0 ** l, f32) for l in range(11)])


# name -> (how the environment is made, the configs to run)
CASES = {
    "a": (("equirect", lambda: random_equirect(64, 32, 11)),
          [config(ggx_samples=16, ggx_mips=3, diffuse_samples=64, diffuse_resolution=8),
           config(ggx_samples=256, ggx_mips=3, diffuse_samples=512, diffuse_resolution=8)]),
    "b": (("equirect", lambda: random_equirect(8, 4, 12)),
          [config(ggx_samples=64, ggx_mips=2, diffuse_samples=128, diffuse_resolution=1),
           config(ggx_samples=64, ggx_mips=2, diffuse_samples=128, diffuse_resolution=3)]),
    "c": (("equirect", lambda: scenes.sky_image(256, 128, seed=7)), [config()]),
    "d": (("raw", bright_corner_cube),
          [config(ggx_samples=64, ggx_mips=3, diffuse_samples=128, diffuse_resolution=5)]),
}
DIFFUSE_SUBSET = 2000      # of case c's 6 * 256 * 256 diffuse texels


def levels_of(cfg, N):
    """The launches of one pt_env_filter: (which, mip, kind, n, samples, roughness, bias, texels), texels = (face, x, y) arrays."""
    mips = cfg.ggx_mips or er.reference_ggx_mips(N)
    out = []
    for i, n in enumerate(er.ggx_level_sizes(N, mips)):
        out.append((abi.ENV_FILTER_GGX, i, er.GGX, n, cfg.ggx_samples, er.mip_to_roughness(i, mips), cfg.ggx_mip_bias, er.all_texels(n)))
    n = cfg.diffuse_resolution
    texels = er.all_texels(n)
    if 6 * n * n > 4 * DIFFUSE_SUBSET:
        pick = np.sort(np.random.default_rng(2000).choice(6 * n * n, DIFFUSE_SUBSET, replace=False))
        texels = tuple(t[pick] for t in texels)
    out.append((abi.ENV_FILTER_DIFFUSE, 0, er.DIFFUSE, n, cfg.diffuse_samples, f32(0), cfg.diffuse_mip_bias, texels))
    return out
