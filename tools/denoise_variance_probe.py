#!/usr/bin/env python3
"""Run ON THE GPU BOX: what pt_denoise_variance costs at 1920 x 1080 on the 8-spp images of config 3 (the Sponza-class scene) beside
pt_denoise on the same images in the same process, both at their defaults, timed from outside with stream events as
tools/denoise_probe.py does: ROUNDS rounds of the two filters in turn, each the median of CALLS enqueues after WARMUP warm-ups.  The
bytes suggest a ratio near 1.2: a tap moves 36 B through L2 where pt_denoise's moves 32 B, and a 9-tap prefilter pass comes on top.
Both filters are instantiations of one kernel family (gltf_renderer_amd/csrc/denoise.hip: k_at_prepare, k_at_prefilter, k_at_pass,
k_at_pass_lds), so a change there is measured on both by one run.  MIPT_LIBRARY (gltf_renderer_amd/renderer.py) times another build of the
library in the same way.
usage: python tools/denoise_variance_probe.py [--calls 30] [--rounds 2] [--size 1920 1080] [--iterations 5] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--iterations", type=int, nargs="+", default=[5])
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if a.calls < 20:
        raise SystemExit("denoise_variance_probe.py: --calls must be >= 20")

    import torch
    from gltf_renderer_amd import abi, scenes
    from gltf_renderer_amd.renderer import Renderer
    if not torch.cuda.is_available():
        raise SystemExit("denoise_variance_probe.py: no GPU, nothing measured")

    s = scenes.sponza_class()
    s.width, s.height = a.size
    w, h = a.size
    r = Renderer(0)
    hd = s.upload(r)
    r.build_accel()
    out, alb, nd, var, den = (r.create_output(w, h) for _ in range(5))
    r.set_aov(alb, nd)
    r.set_variance(var)
    st = abi.PtSettings.from_buffer_copy(bytes(s.settings))
    st.reset = 1
    r.set_samples_per_trace(8)
    r.trace(st, s.execute_params(0, env_handle=hd["env"]), out)            # the 8-spp images
    torch.cuda.synchronize()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    res = {"width": w, "height": h, "calls": a.calls, "warmup": a.warmup, "library": os.environ.get("MIPT_LIBRARY", ""), "rounds": []}
    for it in a.iterations:
        old, new = abi.PtDenoiseConfig.default(), abi.PtDenoiseVarianceConfig.default()
        old.iterations = new.iterations = it
        for k in range(a.rounds):
            m_old = timed(lambda: r.denoise(out, alb, nd, out=den, config=old))
            m_new = timed(lambda: r.denoise_variance(out, alb, nd, var, samples=8, out=den, config=new))
            res["rounds"].append({"iterations": it, "denoise_ms": [round(x, 4) for x in m_old], "denoise_variance_ms": [round(x, 4) for x in m_new],
                                  "ratio": round(m_new[0] / m_old[0], 3)})
            print("%dx%d, %d pass(es), round %d: pt_denoise median %.4f ms (min %.4f, max %.4f), pt_denoise_variance median %.4f ms (min %.4f, "
                  "max %.4f), ratio %.3f" % ((w, h, it, k) + m_old + m_new + (m_new[0] / m_old[0],)), flush=True)
    filtered = r.readback(den)
    res["checksum"] = "%08x" % (int(filtered.view("uint32").astype("uint64").sum()) & 0xffffffff)      # two builds that must agree in bits
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    r.close()


if __name__ == "__main__":
    main()
