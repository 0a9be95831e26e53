#!/usr/bin/env python3
"""Rehearse pt_denoise's and pt_denoise_variance's kernels WITHOUT a GPU: the kernel source of gltf_renderer_amd/csrc/denoise.hip (everything
in its first anonymous namespace) is compiled for the host with g++ -ffp-contract=off behind a few lines that stand in for the HIP
built-ins, run block by block and thread by thread, and compared with tests/denoise_ref.py and tests/denoise_variance_ref.py on the cases of
tests/test_gpu_denoise.py and tests/test_gpu_denoise_variance.py.  What this shows: indexing, tap order, validity, the tiles' counts.  What
it cannot show: the device's expf, any time, and the LDS-staged kernel of the variance filter's passes at spacings 1 and 2, which needs a
block's lanes side by side (every pass runs the direct kernel here; the staged one has to parse, no more, and gives its bits on the MI355X).
It prints, per filter and case, E32, the host build's distance from the float64 restatement, their ratio, the share of values bit-equal to
the float32 restatement, and the CRC-32 of the host build's image: a change to the kernels that should change no bit changes no CRC.
usage: python tools/denoise_host_rehearsal.py"""
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import denoise_ref as dr  # noqa: E402
from tests import denoise_variance_ref as dv  # noqa: E402

f32 = np.float32

PRELUDE = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
struct float4 { float x, y, z, w; }; struct float3 { float x, y, z; };
struct dim3 { unsigned x, y, z; };
static dim3 blockIdx, threadIdx;
static inline float4 make_float4(float x, float y, float z, float w) { return {x, y, z, w}; }
static inline float3 make_float3(float x, float y, float z) { return {x, y, z}; }
static inline void __syncthreads() {}
using std::isfinite;
#define PT_TILE 16
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static
"""

DRIVER = r"""template <class F> void grid_run(uint32_t w, uint32_t h, F f) {
    for (unsigned by = 0; by < (h + AT_BY - 1) / AT_BY; by++) for (unsigned bx = 0; bx < (w + AT_BX - 1) / AT_BX; bx++) {
        blockIdx = {bx, by, 0};
        for (unsigned ty = 0; ty < AT_BY; ty++) for (unsigned tx = 0; tx < AT_BX; tx++) { threadIdx = {tx, ty, 0}; f(); }
    }
}
// in.bin: w h iterations demodulate npow has_counts samples (int32), sigma_depth sigma (float32), color, albedo, nd, VAR: variance, counts
template <bool VAR> int run(const char* in, const char* to) {
    FILE* f = fopen(in, "rb"); int32_t hd[7]; float sg[2];
    if (fread(hd, 4, 7, f) != 7 || fread(sg, 4, 2, f) != 2) return 2;
    uint32_t w = hd[0], h = hd[1]; size_t n = (size_t)w * h;
    const uint32_t tiles_x = (w + PT_TILE - 1) / PT_TILE, tiles = tiles_x * ((h + PT_TILE - 1) / PT_TILE);
    std::vector<float4> color(n), albedo(n), nd(n), var(n), out(n), ping(n), pong(n), guide(n);
    std::vector<float> vt(n);
    std::vector<uint32_t> counts(tiles);
    if (fread(color.data(), 16, n, f) != n || fread(albedo.data(), 16, n, f) != n || fread(nd.data(), 16, n, f) != n) return 2;
    if (VAR && fread(var.data(), 16, n, f) != n) return 2;
    if (hd[5] && fread(counts.data(), 4, tiles, f) != tiles) return 2;
    fclose(f);
    memset(out.data(), 0x55, n * 16);
    grid_run(w, h, [&] { k_at_prepare<VAR>(color.data(), albedo.data(), nd.data(), var.data(), w, h, tiles_x, hd[5] ? counts.data() : nullptr, (uint32_t)hd[6], hd[3] != 0, ping.data(), guide.data()); });
    float4 *src = ping.data(), *dst = pong.data();
    for (int i = 0; i < hd[2]; i++) {
        AtPass a; a.S = src; a.G = guide.data(); a.vt = vt.data(); a.dst = dst; a.w = w; a.h = h; a.step = 1 << i; a.normal_squarings = hd[4];
        a.zk = sg[0] * (float)a.step; const float sig = VAR ? sg[1] : sg[1] * ldexpf(1.0f, -i); a.sig2 = sig * sig; a.color_on = sg[1] != 0.0f;
        a.color = color.data(); a.albedo = albedo.data(); a.out = out.data(); a.demodulate = hd[3] != 0;
        const bool last = i == hd[2] - 1;
        if (VAR) grid_run(w, h, [&] { k_at_prefilter(src, guide.data(), w, h, vt.data()); });
        grid_run(w, h, [&] { if (last) k_at_pass<VAR, true>(a); else k_at_pass<VAR, false>(a); });
        float4* t = src; src = dst; dst = t;
    }
    f = fopen(to, "wb"); fwrite(out.data(), 16, n, f); fclose(f);
    return 0;
}
template __global__ void k_at_pass_lds<true, false, 1>(const AtPass);       // has to parse, no more
int main(int argc, char** argv) { return argv[1][0] == 'v' ? run<true>(argv[2], argv[3]) : run<false>(argv[2], argv[3]); }
"""


def build(tmp):
    src = open(os.path.join(ROOT, "gltf_renderer_amd", "csrc", "denoise.hip")).read()
    a = src.index("namespace {") + len("namespace {")
    b = src.index("}  // namespace\n")
    cpp = os.path.join(tmp, "denoise_host.cpp")
    with open(cpp, "w") as f:
        f.write(PRELUDE + src[a:b] + DRIVER)
    exe = os.path.join(tmp, "denoise_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-o", exe, cpp])
    return exe


def run(exe, tmp, images, tile_samples, samples, cfg, sigma):
    """images: color, albedo, nd and, for the variance filter, variance"""
    h, w = images[0].shape[:2]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([w, h, cfg.iterations, cfg.demodulate, cfg.normal_power_log2, tile_samples is not None, samples], np.int32).tobytes())
        f.write(np.array([cfg.sigma_depth, sigma], f32).tobytes())
        for x in images:
            f.write(np.ascontiguousarray(x, f32).tobytes())
        if tile_samples is not None:
            f.write(np.ascontiguousarray(tile_samples, np.uint32).tobytes())
    subprocess.check_call([exe, "variance" if len(images) == 4 else "plain", fin, fout])
    return np.fromfile(fout, f32).reshape(h, w, 4)


def tile_pattern(w, h):
    """Counts 0, 1, 2 and 64 over the tile grid, in turn."""
    ty, tx = (h + dv.TILE - 1) // dv.TILE, (w + dv.TILE - 1) // dv.TILE
    return np.array([0, 1, 2, 64], np.uint32)[np.arange(ty * tx) % 4].reshape(ty, tx)


def report(head, color, cfg, sigma, direct, ref32, ref64, valid):
    """One printed line; is the case good"""
    e32, err = dr.rel_error(ref32, ref64, valid), dr.rel_error(direct, ref64, valid)
    keep = np.array_equal(direct[~valid].view(np.uint32), color[~valid].view(np.uint32)) and \
        np.array_equal(direct[..., 3].view(np.uint32), color[..., 3].view(np.uint32))
    print("%s it %d dem %d pow %2d %s: E32 %.2e host %.2e ratio %.2f, == ref32 in %3.0f %%, invalid and alpha kept %s, crc %08x"
          % (head, cfg.iterations, cfg.demodulate, cfg.normal_power_log2, sigma, e32, err, err / e32 if e32 else 0.0,
             100.0 * (direct[valid][:, :3] == ref32[valid][:, :3]).mean() if valid.any() else 100.0, keep, zlib.crc32(direct.tobytes())))
    return keep and err <= 8 * e32


SIZES = ((72, 40), (17, 33), (5, 3), (1, 1), (200, 90))


def main():
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        print("pt_denoise")
        variants = [dr.Config(), dr.Config(demodulate=0), dr.Config(sigma_color=0), dr.Config(normal_power_log2=0), dr.Config(iterations=1),
                    dr.Config(iterations=2), dr.Config(iterations=6, normal_power_log2=10, sigma_depth=0.5, sigma_color=4.0)]
        for (w, h) in SIZES:
            sc = dr.scene(w, h, spp=8, seed=3)
            sc["color"][..., 3] = np.random.default_rng(w * 1000 + h).random((h, w)).astype(f32)
            for cfg in (variants if (w, h) == (72, 40) else [dr.Config(iterations=6), dr.Config(iterations=3)]):
                args = (sc["color"], sc["albedo"], sc["normal_depth"])
                ref64, valid = dr.denoise(*args, cfg, np.float64)
                ref32, _ = dr.denoise(*args, cfg, f32)
                direct = run(exe, tmp, args, None, 0, cfg, cfg.sigma_color)
                bad += not report("%3dx%-3d" % (w, h), sc["color"], cfg, "sc %.1f" % cfg.sigma_color, direct, ref32, ref64, valid)
        print("pt_denoise_variance")
        variants = [dv.Config(), dv.Config(demodulate=0), dv.Config(sigma_variance=0), dv.Config(normal_power_log2=0), dv.Config(iterations=1),
                    dv.Config(iterations=2), dv.Config(iterations=6, normal_power_log2=10, sigma_depth=0.5, sigma_variance=16.0)]
        for (w, h) in SIZES:
            for tiled in (False, True):
                ts = tile_pattern(w, h) if tiled else None
                counts = dv.pixel_counts(ts, w, h) if tiled else np.full((h, w), 8, np.int64)
                sc = dv.scene(w, h, counts=counts, seed=3)
                sc["color"][..., 3] = np.random.default_rng(w * 1000 + h).random((h, w)).astype(f32)
                for cfg in (variants if (w, h) == (72, 40) else [dv.Config(iterations=6), dv.Config(iterations=3)]):
                    args = (sc["color"], sc["albedo"], sc["normal_depth"], sc["variance"])
                    ref64, valid = dv.denoise_variance(*args, counts, cfg, np.float64)
                    ref32, _ = dv.denoise_variance(*args, counts, cfg, f32)
                    direct = run(exe, tmp, args, ts, 8, cfg, cfg.sigma_variance)
                    bad += not report("%3dx%-3d %s" % (w, h, "tiles" if tiled else "8 spp"), sc["color"], cfg, "sv %4.1f" % cfg.sigma_variance,
                                      direct, ref32, ref64, valid)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
