#!/usr/bin/env python3
"""Rehearse pt_denoise's kernels WITHOUT a GPU: the kernel source of gltf_renderer_amd/csrc/denoise.hip (everything in its anonymous
namespace) is compiled for the host with g++ -ffp-contract=off behind a few lines that stand in for the HIP
built-ins, run block by block and thread by thread, and compared with tests/denoise_ref.py on the cases of tests/test_gpu_denoise.py.
What this shows: indexing, tap order, validity.  What it cannot show: the device's expf, and any time.  It prints, per case, E32, the host build's distance from the float64
restatement, their ratio, and the share of values bit-equal to the float32 restatement.
usage: python tools/denoise_host_rehearsal.py"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import denoise_ref as dr  # noqa: E402

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
using std::isfinite;
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
"""

DRIVER = r"""template <class F> void grid_run(uint32_t w, uint32_t h, F f) {
    for (unsigned by = 0; by < (h + DN_BY - 1) / DN_BY; by++) for (unsigned bx = 0; bx < (w + DN_BX - 1) / DN_BX; bx++) {
        blockIdx = {bx, by, 0};
        for (unsigned ty = 0; ty < DN_BY; ty++) for (unsigned tx = 0; tx < DN_BX; tx++) { threadIdx = {tx, ty, 0}; f(); }
    }
}
int main(int argc, char** argv) {
    // in.bin: w h iterations demodulate npow sigma_depth sigma_color (as int32/float32) then color, albedo, nd
    FILE* f = fopen(argv[1], "rb"); int32_t hd[5]; float sg[2];
    if (fread(hd, 4, 5, f) != 5 || fread(sg, 4, 2, f) != 2) return 2;
    uint32_t w = hd[0], h = hd[1]; size_t n = (size_t)w * h;
    std::vector<float4> color(n), albedo(n), nd(n), out(n), ping(n), pong(n), guide(n);
    if (fread(color.data(), 16, n, f) != n || fread(albedo.data(), 16, n, f) != n || fread(nd.data(), 16, n, f) != n) return 2;
    fclose(f);
    memset(out.data(), 0x55, n * 16);
    grid_run(w, h, [&] { k_dn_prepare(color.data(), albedo.data(), nd.data(), w, h, hd[3] != 0, ping.data(), guide.data()); });
    float4 *src = ping.data(), *dst = pong.data();
    for (int i = 0; i < hd[2]; i++) {
        DnPass a; a.S = src; a.G = guide.data(); a.dst = dst; a.w = w; a.h = h; a.step = 1 << i; a.normal_squarings = hd[4];
        a.zk = sg[0] * (float)a.step; const float sig = sg[1] * ldexpf(1.0f, -i); a.sig2 = sig * sig; a.color_on = sg[1] != 0.0f;
        a.color = color.data(); a.albedo = albedo.data(); a.out = out.data(); a.demodulate = hd[3] != 0;
        const bool last = i == hd[2] - 1;
        grid_run(w, h, [&] { if (last) k_dn_pass<true>(a); else k_dn_pass<false>(a); });
        float4* t = src; src = dst; dst = t;
    }
    f = fopen(argv[2], "wb"); fwrite(out.data(), 16, n, f); fclose(f);
    return 0;
}
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


def run(exe, tmp, color, albedo, nd, cfg):
    h, w = color.shape[:2]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([w, h, cfg.iterations, cfg.demodulate, cfg.normal_power_log2], np.int32).tobytes())
        f.write(np.array([cfg.sigma_depth, cfg.sigma_color], f32).tobytes())
        for x in (color, albedo, nd):
            f.write(np.ascontiguousarray(x, f32).tobytes())
    subprocess.check_call([exe, fin, fout])
    return np.fromfile(fout, f32).reshape(h, w, 4)


def main():
    variants = [dr.Config(), dr.Config(demodulate=0), dr.Config(sigma_color=0), dr.Config(normal_power_log2=0), dr.Config(iterations=1),
                dr.Config(iterations=2), dr.Config(iterations=6, normal_power_log2=10, sigma_depth=0.5, sigma_color=4.0)]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for (w, h) in ((72, 40), (17, 33), (5, 3), (1, 1), (200, 90)):
            sc = dr.scene(w, h, spp=8, seed=3)
            sc["color"][..., 3] = np.random.default_rng(w * 1000 + h).random((h, w)).astype(f32)
            for cfg in (variants if (w, h) == (72, 40) else [dr.Config(iterations=6), dr.Config(iterations=3)]):
                args = (sc["color"], sc["albedo"], sc["normal_depth"], cfg)
                ref64, valid = dr.denoise(*args, np.float64)
                ref32, _ = dr.denoise(*args, f32)
                direct = run(exe, tmp, *args)
                e32, err = dr.rel_error(ref32, ref64, valid), dr.rel_error(direct, ref64, valid)
                keep = np.array_equal(direct[~valid].view(np.uint32), sc["color"][~valid].view(np.uint32)) and \
                    np.array_equal(direct[..., 3].view(np.uint32), sc["color"][..., 3].view(np.uint32))
                ok = keep and err <= 8 * e32
                bad += not ok
                print("%3dx%-3d it %d dem %d pow %2d sc %.1f: E32 %.2e host %.2e ratio %.2f, == ref32 in %3.0f %%, invalid and alpha kept %s"
                      % (w, h, cfg.iterations, cfg.demodulate, cfg.normal_power_log2, cfg.sigma_color, e32, err, err / e32 if e32 else 0.0,
                         100.0 * (direct[valid][:, :3] == ref32[valid][:, :3]).mean() if valid.any() else 100.0, keep))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
