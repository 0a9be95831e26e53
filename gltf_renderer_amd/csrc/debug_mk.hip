// debug_mk.hip -- the device side of the test hooks (pt_debug_*, mipt_debug.hip) that run what the megakernel runs, compiled as pt_kernel.hip
// is (same Makefile flags, no PT_LUT_LDS): the per-lane query kernels with every table in global memory (pt_debug_kernels.h), the megakernel's
// traversal driver on caller-supplied rays, and the kernels' math routines.  No frame runs anything in this file.
#include "pt_debug_kernels.h"
#include "dev_buf.h"
#include "mipt_debug.h"

namespace pt {

DebugQueryLaunch debug_queries_mk() { return kDebugQueryLaunch; }

// Test hook (pt_debug_intersect): the product's traversal on caller-supplied rays, one ray per lane -- what TraceRay / TraceShadowRay find,
// without the shading around them.  rays: 8 floats each (origin, tmin, direction, tmax); out: 8 floats each (committed, t, u, v, instance,
// primitive, front face, transmission).
__global__ __launch_bounds__(kBlock) void k_debug_intersect(SceneRec sc, const float* __restrict__ rays, uint32_t n, uint32_t rf, int mode, float* __restrict__ out) {
    __shared__ int s_stack[kStackLds * kBlock];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float* q = rays + (size_t)i * 8;
    Ray r; r.o = v3(q[0], q[1], q[2]); r.tmin = q[3]; r.d = v3(q[4], q[5], q[6]); r.tmax = q[7];
    HitRec hit; LaneStats st = {0, 0, 0, 0, 0};
    float transmission = (mode == 1 && (rf & RF_FORCE_NON_OPAQUE)) ? 1.0f : 0.0f;
    const bool got = traverse<false>(sc, s_stack + threadIdx.x, r, rf, 0xff, mode, hit, transmission, st);
    float* o = out + (size_t)i * 8;
    const bool have = got && hit.tri >= 0;
    o[0] = got ? 1.0f : 0.0f; o[1] = have ? hit.t : 0.0f; o[2] = have ? hit.u : 0.0f; o[3] = have ? hit.v : 0.0f;
    o[4] = have ? (float)sc.tris[hit.tri].inst : -1.0f; o[5] = have ? (float)sc.tris[hit.tri].prim : -1.0f; o[6] = (have && hit.front) ? 1.0f : 0.0f;
    o[7] = transmission;
}
void launch_debug_intersect(const SceneRec& sc, const float* d_rays, uint32_t n, uint32_t rf, int mode, float* d_out, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_debug_intersect, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, sc, d_rays, n, rf, mode, d_out);
}

// Test hook (pt_debug_math): the kernels' own math routines on caller-supplied arguments, for the bit-for-bit comparison with the oracle's.
// op: 0 atan2(a, b)  1 pow(a, b)  2 exp(a)  3 log2(a)  4 exp2(a)  5 sin(a)  6 cos(a)  7 a / b by fdiv  8 pow5(a)
__global__ __launch_bounds__(256) void k_debug_math(int op, const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float x = a[i], y = b[i];
    float r = 0, s, c;
    switch (op) {
        case 0: r = pt_atan2(x, y); break;
        case 1: r = hpow(x, y); break;
        case 2: r = pt_exp(x); break;
        case 3: r = co_log2(x); break;
        case 4: r = co_exp2(x); break;
        case 5: pt_sincos(x, s, c); r = s; break;
        case 6: pt_sincos(x, s, c); r = c; break;
        case 7: r = fdiv(x, y); break;
        case 8: r = hpow5(x); break;
    }
    out[i] = r;
}
}  // namespace pt
// host arrays, no context: 0, or -3 for whatever fails
extern "C" int pt_debug_math(int op, const float* a, const float* b, float* out, uint32_t n) {
    if (n == 0) return 0;
    const size_t bytes = (size_t)n * 4;
    pt::TempBuf da, db, dc;
    if (da.alloc(bytes) != hipSuccess || db.alloc(bytes) != hipSuccess || dc.alloc(bytes) != hipSuccess) return -3;
    if (hipMemcpy(da.ptr, a, bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(db.ptr, b, bytes, hipMemcpyHostToDevice) != hipSuccess) return -3;
    hipLaunchKernelGGL(pt::k_debug_math, dim3((n + 255) / 256), dim3(256), 0, nullptr, op, da.as<const float>(), db.as<const float>(), dc.as<float>(), n);
    return hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, dc.ptr, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}
