#!/usr/bin/env python3
"""Decode the reference's Resources/Sheen_E.exr into the two data files the repo ships.

The file is a 16x16 single-channel HALF scanline EXR whose only chunk is stored raw
(chunk size field = 512 = 16*16*2): little-endian halfs at
byte offset 293, row = v = alpha, column = u = cos_theta.  Loaded by the reference at
Source/GpuResources.cpp:72-132 and sampled by SheenE (Source/Shaders/Bsdf.hlsli:204-208).

Input: the upstream file, stored unchanged as tests/golden/sheen_e.exr (or a path given as
the first argument).  Its two outputs are committed data:
  tests/golden/sheen_e_16x16.npy            (fixture the oracle tests pin against)
  gltf_renderer_amd/data/sheen_e_16x16.f32  (table pt_create loads; 256 little-endian f32)
The LUT is (c) Dassault Systemes, CC-BY-SA (see Resources/Sheen_E_LICENCE.txt upstream).
"""
import sys
import numpy as np

src = sys.argv[1] if len(sys.argv) > 1 else "tests/golden/sheen_e.exr"
raw = open(src, "rb").read()
assert len(raw) == 805, len(raw)
lut = np.frombuffer(raw[293:293 + 512], dtype="<f2").astype(np.float32).reshape(16, 16)
np.save("tests/golden/sheen_e_16x16.npy", lut)
lut.tofile("gltf_renderer_amd/data/sheen_e_16x16.f32")
print("min %.3e max %.4f" % (lut.min(), lut.max()))
