#!/bin/bash
# Build variants/libmipt_<name>.so: the library with extra -D tuning macros on the path-tracing translation units (A/B runs on the
# GPU box with tools/bench_variants.sh).  usage: [ONLY="pt_wavefront ..."] tools/build_variant.sh <name> [-DFOO=1 ...]
# ONLY: the files that get the macros (default: all five); -DPT_TIMING needs ONLY=pt_wavefront, the one file that defines its counters.
set -e
NAME=$1; shift
cd "$(dirname "$0")/../gltf_renderer_amd/csrc"
mkdir -p ../../variants /tmp/variant_$NAME
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -Wno-unused-variable -Wno-unused-value -I../../include"
for f in pt_wavefront pt_kernel debug_wf debug_mk accel; do      # (the hooks' files run the code of the two before them: same macros)
  X="-ffp-contract=off"; [ $f != accel ] && X="-fno-slp-vectorize -ffp-contract=off"      # as in the Makefile: no contraction anywhere, the path-tracing kernels also without the SLP vectoriser
  D="$@"; [ -n "$ONLY" ] && ! echo " $ONLY " | grep -q " $f " && D=""
  /opt/rocm/bin/hipcc $FLAGS $D $X -c $f.hip -o /tmp/variant_$NAME/$f.o &
done
wait
# everything else the library links, as the Makefile lists and builds it
REST=$(make -s print-objs | tr ' ' '\n' | grep -vxE '(pt_wavefront|pt_kernel|debug_wf|debug_mk|accel)\.o' | tr '\n' ' ')
make -s $REST
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o ../../variants/libmipt_$NAME.so /tmp/variant_$NAME/pt_wavefront.o /tmp/variant_$NAME/pt_kernel.o /tmp/variant_$NAME/debug_wf.o /tmp/variant_$NAME/debug_mk.o /tmp/variant_$NAME/accel.o \
  $REST -ldl
echo built variants/libmipt_$NAME.so
