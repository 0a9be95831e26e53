"""pt_env_filter (include/mipt.h) on the MI355X: the kernels of csrc/envfilter.hip against tests/envfilter_ref.py, on the cases of
tests/envfilter_cases.py (the smallest shapes at which they can still go wrong), then what the call must leave alone and how it behaves.

The bar, for every texel of every level (case c's 256^2 diffuse cube: a fixed subset of 2000), against the FLOAT64 restatement:
    |gpu - ref64| <= (one RGBA16F rounding of the value) + K * E32 * (the largest tap the texel fetched)
E32 is the float32 restatement's largest distance from the float64 one on that level, as a share of the largest tap (computed here by the
same tests/envfilter_ref.py e32() that tests/test_envfilter_host.py records: 0 to 17 x 2^-24 on these cases).  The kernels compute the
float32 text, so their distance from float64 is the restatement's own, except where the device's sin / cos (through double, but another
libm) and numpy's part in a last bit.  Measured once on the MI355X, max over the texels of a level of (|gpu - ref64| - rounding) /
(E32 * tap): see MEASURED below; K is set from that, with a small margin.
"""
import ctypes as C

import numpy as np
import pytest

from gltf_renderer_amd import abi, scenes
from tests import envfilter_cases as ec
from tests import envfilter_ref as er
from tests import hooks

pytestmark = pytest.mark.gpu

f16, f32, f64 = np.float16, np.float32, np.float64
MEASURED = ("one MI355X: every stored texel of every level of the four cases equals the float32 restatement's rounded to half, bit for bit; "
            "(|gpu - ref64| - rounding) / (E32 tap) is 0 on 22 of the 24 levels, 0.036 on case c's GGX level 1 and 0.118 on its diffuse cube")
K = 1.25      # a quarter over the 1 that bit-equality with the float32 restatement needs: room for a libm whose double sin / cos part in a last bit


def make_env(r, how, make):
    if how == "raw":
        cube = make()
        out = C.c_int(-1)
        rc = hooks.lib().pt_debug_env_create_raw(r.h, cube.shape[1], cube.ctypes.data, ec.unit_pyramid().ctypes.data, C.addressof(out))
        assert rc == 0, rc
        return out.value
    return r.env_create(make())


@pytest.fixture(scope="module")
def r():
    from gltf_renderer_amd.renderer import Renderer
    r = Renderer(0)
    yield r
    r.close()


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_every_texel_is_within_the_bar_of_the_float64_restatement(r, name):
    (how, make), configs = ec.CASES[name]
    env = make_env(r, how, make)
    N, cube, _ = r.env_read(env)
    assert N == {"a": 9, "b": 2, "c": 33, "d": 5}[name]
    chain = er.chain_from_mip0(cube)
    worst = 0.0
    for cfg in configs:
        r.env_filter(env, cfg)
        info = r.env_filter_info(env)
        levels = ec.levels_of(cfg, N)
        assert info.ggx_mips == len(levels) - 1 and info.ggx_resolution == N and info.diffuse_resolution == cfg.diffuse_resolution
        for which, mip, kind, n, S, a, bias, tex in levels:
            texels, _ = r.env_filter_read(env, which, mip)
            assert texels.shape == (6, n, n, 4) and (texels[..., 3] == 0).all()                    # alpha as the cube's mips write it
            if which == abi.ENV_FILTER_GGX:
                assert f32(info.ggx_roughness[mip]) == a
            gpu = er.half_rgb(texels)[tex[0], tex[2], tex[1]].astype(f64)
            E, v32, v64, big = er.e32(chain, kind, n, tex, S, a, bias)
            assert np.isfinite(gpu).all() and np.isfinite(v64).all()
            rounding = er.half_rounding(np.maximum(np.abs(gpu), np.abs(v64)))
            err = np.abs(gpu - v64)
            unit = E * big[:, None]
            with np.errstate(all="ignore"):
                ratio = np.where(err > rounding, (err - rounding) / unit, 0.0)
            exact = float((gpu == er.to_half(v32)).all(axis=1).mean())
            print("case %s which %d mip %d n %d S %d a %.4f: E32 %.3e, (|gpu - ref64| - rounding) / (E32 tap) max %.3f, texels equal to the "
                  "float32 restatement's half %.4f" % (name, which, mip, n, S, a, E, np.nanmax(ratio) if E > 0 else 0.0, exact))
            worst = max(worst, float(np.nanmax(ratio)) if E > 0 else 0.0)
            assert (err <= rounding + K * unit).all(), (name, which, mip, float((err - rounding - K * unit).max()))
    print("case %s: worst ratio %.3f (K = %.2f)" % (name, worst, K))
    r.env_destroy(env)


def test_the_level_of_roughness_zero_is_the_cubes_mip_zero_within_one_half_rounding(r):
    for name in ("a", "c"):
        (how, make), configs = ec.CASES[name]
        env = make_env(r, how, make)
        N, cube, _ = r.env_read(env)
        r.env_filter(env, configs[0])
        texels, _ = r.env_filter_read(env, abi.ENV_FILTER_GGX, 0)
        got, own = er.half_rgb(texels).astype(f64), er.half_rgb(cube).astype(f64)
        assert (np.abs(got - own) <= 2 * er.half_rounding(np.maximum(np.abs(got), np.abs(own)))).all()
        r.env_destroy(env)


def test_the_tracer_is_untouched():
    """pt_env_read and an accumulated pt_trace image under FLAG_ENVIRONMENT_MAP | FLAG_ENVIRONMENT_MIS are bit-identical before and after
    pt_env_filter, and the ray counts are equal."""
    from gltf_renderer_amd.renderer import Renderer
    s = scenes.test_scene(48, 16)
    assert s.settings.flags & abi.FLAG_ENVIRONMENT_MAP and s.settings.flags & abi.FLAG_ENVIRONMENT_MIS
    r = Renderer(0)
    h = s.upload(r)

    def render():
        out = r.create_output(s.width, s.height)
        r.reset_stats()
        st = abi.PtSettings.from_buffer_copy(bytes(s.settings))
        st.reset = 1
        for f in range(4):
            r.trace(st, s.execute_params(f, env_handle=h["env"]), out)
            st.reset = 0
        img = r.readback(out)
        return img, r.stats().rays

    n0, cube0, pyr0 = r.env_read(h["env"])
    img0, rays0 = render()
    r.env_filter(h["env"], ec.config(ggx_samples=32, diffuse_samples=32, diffuse_resolution=16))
    n1, cube1, pyr1 = r.env_read(h["env"])
    img1, rays1 = render()
    assert n0 == n1 and np.array_equal(cube0, cube1) and np.array_equal(pyr0.view(np.uint32), pyr1.view(np.uint32))
    assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32)) and rays0 == rays1 and rays0 > 0
    assert np.isfinite(img0).all() and img0[..., :3].max() > 0
    r.close()


def test_life_cycle_and_arguments():
    from gltf_renderer_amd.renderer import Renderer
    r = Renderer(0)
    L = r.L
    img = ec.random_equirect(64, 32, 3)                                      # N = 9: four cube levels
    env = r.env_create(img)
    P = abi.PtEnvFilterConfig
    nan, inf = float("nan"), float("inf")
    info, n, dev = abi.PtEnvFilterInfo(), C.c_int(-7), C.c_void_p(5)
    # before the first filter
    assert L.pt_env_filter_info_get(r.h, env, C.byref(info)) == -6
    assert L.pt_env_filter_read(r.h, env, 0, 0, C.byref(n), None, C.byref(dev)) == -6 and (n.value, dev.value) == (-7, 5)
    # a bad handle
    for bad in (-1, env + 1, 1000):
        assert L.pt_env_filter(r.h, bad, None) == -4 and L.pt_env_filter_info_get(r.h, bad, C.byref(info)) == -4
        assert L.pt_env_filter_read(r.h, bad, 0, 0, C.byref(n), None, None) == -4
    # every range limit: the value outside is refused with nothing changed, the limit itself is taken
    small = dict(ggx_samples=4, ggx_mips=2, diffuse_samples=4, diffuse_resolution=2)
    refused = [dict(ggx_samples=0), dict(ggx_samples=4097), dict(ggx_samples=-1), dict(ggx_mip_bias=nan), dict(ggx_mip_bias=inf), dict(ggx_mip_bias=-inf),
               dict(ggx_mips=-1), dict(ggx_mips=5), dict(diffuse_samples=0), dict(diffuse_samples=4097), dict(diffuse_mip_bias=nan),
               dict(diffuse_mip_bias=inf), dict(diffuse_resolution=0), dict(diffuse_resolution=1025)]
    for kw in refused:
        assert L.pt_env_filter(r.h, env, C.byref(ec.config(**dict(small, **kw)))) == -1, kw
        assert L.pt_env_filter_info_get(r.h, env, C.byref(info)) == -6, kw                           # still nothing there
    r.env_filter(env, ec.config(**small))
    first = r.env_filter_info(env)
    assert (first.ggx_resolution, first.ggx_mips, first.diffuse_resolution) == (9, 2, 2) and list(first.ggx_roughness)[:3] == [0.0, 1.0, 0.0]
    kept, _ = r.env_filter_read(env, 1, 0)
    for kw in refused:
        assert L.pt_env_filter(r.h, env, C.byref(ec.config(**dict(small, **kw)))) == -1, kw
    again = r.env_filter_info(env)
    assert bytes(again) == bytes(first) and np.array_equal(r.env_filter_read(env, 1, 0)[0], kept)    # a refusal changed nothing
    for kw in (dict(ggx_samples=1), dict(ggx_samples=4096, ggx_mips=1, diffuse_resolution=1), dict(ggx_mips=4), dict(diffuse_samples=1),
               dict(diffuse_samples=4096, diffuse_resolution=1), dict(diffuse_resolution=1024, diffuse_samples=1), dict(ggx_mip_bias=-50.0, diffuse_mip_bias=50.0)):
        r.env_filter(env, ec.config(**dict(small, **kw)))
    # a chain of one level has roughness 0
    r.env_filter(env, ec.config(**dict(small, ggx_mips=1)))
    one = r.env_filter_info(env)
    assert one.ggx_mips == 1 and all(v == 0.0 for v in one.ggx_roughness)
    # a bad which or mip
    for which, mip in ((2, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1)):
        assert L.pt_env_filter_read(r.h, env, which, mip, C.byref(n), None, None) == -1, (which, mip)
    # twice with different configs: the second one's sizes win
    r.env_filter(env, ec.config(ggx_samples=8, ggx_mips=3, diffuse_samples=8, diffuse_resolution=5))
    a = r.env_filter_info(env)
    ggx_a = [r.env_filter_read(env, 0, m)[0] for m in range(3)]
    r.env_filter(env, ec.config(ggx_samples=8, ggx_mips=4, diffuse_samples=8, diffuse_resolution=3))
    b = r.env_filter_info(env)
    assert (a.ggx_mips, a.diffuse_resolution, b.ggx_mips, b.diffuse_resolution) == (3, 5, 4, 3)
    assert [r.env_filter_read(env, 0, m)[0].shape[1] for m in range(4)] == [9, 4, 2, 1] and r.env_filter_read(env, 1, 0)[0].shape[1] == 3
    assert L.pt_env_filter_read(r.h, env, 0, 4, C.byref(n), None, None) == -1
    assert np.array_equal(r.env_filter_read(env, 0, 0)[0], ggx_a[0])                                # level 0 is a = 0 either way
    assert not np.array_equal(r.env_filter_read(env, 0, 1)[0], ggx_a[1])                            # a = 1/9 now, 1/4 before
    # device_out: the same texels, read through pt_readback (6 n n RGBA16F texels are 3 n n float4)
    for which, mip in ((0, 0), (0, 1), (0, 3), (1, 0)):
        host, dev_ptr = r.env_filter_read(env, which, mip)
        only, dev_again = r.env_filter_read(env, which, mip, host=False)
        assert only is None and dev_again == dev_ptr and dev_ptr
        m = host.shape[1]
        assert (6 * m * m) % 2 == 0
        copy = np.zeros(6 * m * m * 4, np.uint16)
        r._check(L.pt_readback(r.h, C.c_void_p(dev_ptr), 3 * m * m, 1, copy.ctypes.data_as(C.c_void_p)))
        assert np.array_equal(copy.reshape(host.shape), host) and host[..., :3].any()
    # destroy, then create: the handle comes back without the old cubes
    r.env_destroy(env)
    assert L.pt_env_filter(r.h, env, None) == -4 and L.pt_env_filter_info_get(r.h, env, C.byref(info)) == -4
    env2 = r.env_create(img)
    assert env2 == env
    assert L.pt_env_filter_info_get(r.h, env2, C.byref(info)) == -6 and L.pt_env_filter_read(r.h, env2, 0, 0, C.byref(n), None, None) == -6
    r.env_filter(env2, ec.config(**small))
    assert r.env_filter_info(env2).ggx_mips == 2
    r.close()                                                                                       # pt_destroy frees them


def test_on_a_non_blocking_side_stream_the_filter_does_not_wait_and_the_read_does():
    import torch
    from gltf_renderer_amd.renderer import Renderer
    from tests import stream_ballast as sb
    img = ec.random_equirect(64, 32, 4)
    cfg = ec.config(ggx_samples=16, ggx_mips=3, diffuse_samples=16, diffuse_resolution=4)

    def flow(env_):
        r = env_.R()
        e = r.env_create(img)
        r.env_filter(e, cfg)                                                 # the steady state: the cubes at their sizes
        env_.sync()
        ev = env_.ballast()
        r.env_filter(e, cfg)
        env_.open(ev, "pt_env_filter returned (documented asynchronous)")
        _, dev = r.env_filter_read(e, 0, 1, host=False)                      # the pointer alone: no wait either
        env_.open(ev, "pt_env_filter_read without a host buffer returned")
        ggx, _ = r.env_filter_read(e, 0, 1)                                  # synchronises the stream
        if ev is not None:
            assert ev.query(), "pt_env_filter_read returned texels while the ballast in front of the filter was still running"
        diffuse, _ = r.env_filter_read(e, 1, 0)
        return {"ggx": ggx, "diffuse": diffuse}

    want = sb.serial(flow)
    assert want["ggx"][..., :3].any() and want["diffuse"][..., :3].any()
    got = sb.on_streams(flow, [sb.side_stream()])
    torch.cuda.synchronize()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
