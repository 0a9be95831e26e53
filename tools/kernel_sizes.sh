#!/bin/bash
# instruction counts + resource usage of the wavefront kernels (CPU-side, no GPU needed), compiled with the flags the Makefile gives
# the path-tracing kernels and their test hooks (pt_wavefront.hip, wf_passes.hip, pt_kernel.hip, debug_wf.hip, debug_mk.hip, motion.hip).  One line per kernel, sorted by name, so that two listings diff cleanly:
#   tools/kernel_sizes.sh [file.hip] > listing.txt
cd "$(dirname "$0")/../gltf_renderer_amd/csrc"
OUT=$(mktemp /tmp/ks_dev.XXXXXX.s)
trap 'rm -f "$OUT"' EXIT
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-slp-vectorize -ffp-contract=off -I../../include --cuda-device-only -S ${1:-pt_wavefront.hip} -o "$OUT" 2>/dev/null || exit 1
python3 - "$OUT" <<'PY'
import re, sys
cur = None; counts = {}
meta = {}; rec = None
for l in open(sys.argv[1]):
    m = re.match(r'^(_Z\w+):', l)
    if m: cur = m.group(1); counts[cur] = 0
    elif cur and l.startswith('\t') and not l.startswith('\t.') and not l.startswith('\t;'): counts[cur] += 1
    if l.startswith('.Lfunc_end'): cur = None
    m = re.match(r'^\s+(- )?\.(agpr_count|group_segment_fixed_size|name|private_segment_fixed_size|sgpr_count|vgpr_count):\s+(\S+)', l)
    if m:
        if m.group(2) == 'agpr_count' or rec is None or m.group(2) in rec: rec = {}
        rec[m.group(2)] = m.group(3)
        if 'name' in rec: meta[rec['name']] = rec
for name in sorted(meta):
    r = meta[name]
    print("%-72s %6d instr  vgpr %3s  agpr %3s  sgpr %3s  scratch %4s  lds %6s" % (name[:72], counts.get(name, 0), r.get('vgpr_count', '?'), r.get('agpr_count', '0'),
          r.get('sgpr_count', '?'), r.get('private_segment_fixed_size', '?'), r.get('group_segment_fixed_size', '?')))
PY
