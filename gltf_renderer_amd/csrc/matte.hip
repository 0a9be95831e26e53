// matte.hip -- ID mattes (pt_set_matte, include/mipt.h): the entry points that need no path-tracing kernel, and a call's matte_setup.
//
//   pt_matte_id       MurmurHash3_x86_32 (seed 0) of a name, then the exponent fix (pt_matte.h): Cryptomatte's id of a name.  Host only.
//   pt_set_matte      checks and keeps the config and the caller's ids, and marks the device table of ids stale (matte_table_kind = -1).
//   matte_setup       makes that table for the pt_trace that calls it (mipt_api.hip PathtraceScene), which knows the instance and material
//                     tables the ids are for -- unless it stands for this kind and this many rows -- and fills what the matte kernels take.
//   pt_matte_extract  k_matte_extract: one lane per pixel reads the pixel's K / 2 float4 and adds up, in rank order, the coverages whose id
//                     is in the caller's set.  The set (at most 64 ids, fixed on the host) travels in the kernel's arguments: the lanes of
//                     a wave compare against scalar registers, nothing is allocated or copied, and the call is one launch on the stream.
// The record and resolve kernels (k_wf_matte, k_wf_matte_resolve) are stages of the wavefront pipeline and live in wf_passes.hip.
#include "pt_ctx.h"
#include "pt_matte.h"

namespace pt {
namespace {

constexpr int kExtractBlock = 256;

__global__ __launch_bounds__(kExtractBlock) void k_matte_extract(const float4* __restrict__ l0, const float4* __restrict__ l1, const float4* __restrict__ l2,
                                                                 const float4* __restrict__ l3, int ranks, uint32_t pixels, MatteExtractIds ids, int count,
                                                                 float* __restrict__ mask) {
    const uint32_t p = blockIdx.x * kExtractBlock + threadIdx.x;
    if (p >= pixels) return;
    const float4* const layers[4] = {l0, l1, l2, l3};
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (2 * j >= ranks) break;                                      // (uniform)
        const float4 v = layers[j][p];
        const uint32_t ia = __float_as_uint(v.x), ib = __float_as_uint(v.z);
        bool a = false, b = false;
        for (int q = 0; q < count; q++) { a = a || ia == ids.id[q]; b = b || ib == ids.id[q]; }
        if (a) sum = sum + v.y;
        if (b) sum = sum + v.w;
    }
    mask[p] = sum;
}

uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

}  // namespace

void launch_matte_extract(const float4* const layers[4], int ranks, uint32_t pixels, const MatteExtractIds& ids, int count, float* mask, hipStream_t stream) {
    hipLaunchKernelGGL(k_matte_extract, dim3((pixels + kExtractBlock - 1) / kExtractBlock), dim3(kExtractBlock), 0, stream, layers[0], layers[1], layers[2], layers[3],
                       ranks, pixels, ids, count, mask);
}

int matte_setup(pt_ctx* ctx, MatteArgs& matte) {
    const int kind = ctx->matte.kind;
    const size_t rows = kind == PT_MATTE_MATERIAL ? (size_t)ctx->n_materials : ctx->instances.size();
    if (ctx->matte_table_kind != kind || ctx->matte_table_rows != rows) {
        // row i: the caller's id if it gave one, else the id of the default name "instance_<i>" / "material_<i>"
        ctx->matte_table_kind = -1;
        std::vector<uint32_t> table(rows ? rows : 1, 0u);
        for (size_t i = 0; i < rows; i++) {
            if (i < ctx->matte_user_ids.size()) { table[i] = ctx->matte_user_ids[i]; continue; }
            const std::string name = (kind == PT_MATTE_MATERIAL ? "material_" : "instance_") + std::to_string(i);
            table[i] = pt_matte_id(name.data(), name.size());
        }
        // a trace in flight may still read the old table: the copy goes behind it on the stream, a larger table drains it first (DevBuf)
        const size_t bytes = table.size() * 4;
        if (const hipError_t e = ctx->d_matte_ids.reserve(ctx->stream, bytes, bytes + bytes / 2)) return grow_failed(ctx, e, "matte id table: " + std::to_string(bytes) + " bytes");
        if (const hipError_t e = staged_upload(ctx, ctx->d_matte_ids.ptr, table.data(), bytes)) return ctx->fail(PT_ERR_DEVICE, std::string("matte id table: ") + hipGetErrorString(e));
        ctx->matte_table_kind = kind; ctx->matte_table_rows = rows;
    }
    matte.rec = nullptr; matte.ids = ctx->d_matte_ids.as<uint32_t>(); matte.n_ids = (uint32_t)rows;
    matte.kind = kind; matte.ranks = ctx->matte.ranks;
    for (int j = 0; j < 4; j++) matte.layers[j] = j < ctx->matte.ranks / 2 ? (float4*)ctx->matte.layers[j] : nullptr;
    return PT_OK;
}

}  // namespace pt

using namespace pt;

extern "C" {

uint32_t pt_matte_id(const char* name, size_t length) {
    const uint8_t* data = (const uint8_t*)name;
    const uint32_t c1 = 0xcc9e2d51u, c2 = 0x1b873593u;
    uint32_t h = 0;
    const size_t blocks = length / 4;
    for (size_t i = 0; i < blocks; i++) {
        uint32_t k = (uint32_t)data[4 * i] | (uint32_t)data[4 * i + 1] << 8 | (uint32_t)data[4 * i + 2] << 16 | (uint32_t)data[4 * i + 3] << 24;
        k *= c1; k = rotl32(k, 15); k *= c2;
        h ^= k; h = rotl32(h, 13); h = h * 5u + 0xe6546b64u;
    }
    const uint8_t* tail = data + 4 * blocks;
    uint32_t k = 0;
    switch (length & 3) {
        case 3: k ^= (uint32_t)tail[2] << 16; [[fallthrough]];
        case 2: k ^= (uint32_t)tail[1] << 8; [[fallthrough]];
        case 1: k ^= (uint32_t)tail[0]; k *= c1; k = rotl32(k, 15); k *= c2; h ^= k;
    }
    h ^= (uint32_t)length;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return matte_fix(h);
}

int pt_set_matte(pt_ctx* ctx, const pt_matte_config* config, const uint32_t* ids) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!config) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "matte: config is NULL");
    if (!config->enable) {                         // nothing else of a disabled config is looked at; the layers are no longer written
        ctx->matte.enable = 0;
        ctx->restart_pending = true;
        return PT_OK;
    }
    if (config->kind != PT_MATTE_INSTANCE && config->kind != PT_MATTE_MATERIAL) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "matte: kind must be PT_MATTE_INSTANCE or PT_MATTE_MATERIAL");
    if (config->ranks != 2 && config->ranks != 4 && config->ranks != 6 && config->ranks != 8) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "matte: ranks must be 2, 4, 6 or 8");
    for (int j = 0; j < config->ranks / 2; j++)
        if (!config->layers[j]) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "matte: layers[" + std::to_string(j) + "] is NULL (ranks = " + std::to_string(config->ranks) + " needs " + std::to_string(config->ranks / 2) + ")");
    if (config->id_count < 0) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "matte: id_count must be >= 0");
    if (config->id_count > 0 && !ids) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "matte: ids is NULL with id_count = " + std::to_string(config->id_count));
    ctx->matte = *config;
    ctx->matte_user_ids.resize((size_t)config->id_count);
    for (int i = 0; i < config->id_count; i++) ctx->matte_user_ids[(size_t)i] = matte_fix(ids[i]);
    ctx->matte_table_kind = -1;                    // the device table is made anew by the next matte pt_trace (matte_setup)
    ctx->restart_pending = true;
    return PT_OK;
}

int pt_matte_extract(pt_ctx* ctx, const void* const* layers, int ranks, uint32_t width, uint32_t height, const uint32_t* ids, int id_count, void* mask) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!layers || !ids || !mask) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "matte_extract: NULL argument");
    if (ranks != 2 && ranks != 4 && ranks != 6 && ranks != 8) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "matte_extract: ranks must be 2, 4, 6 or 8");
    if (width == 0 || height == 0) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "matte_extract: width and height must be > 0");
    if ((uint64_t)width * height > 0x7fffffffull) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "matte_extract: width * height exceeds 2^31 - 1");
    if (id_count < 1 || id_count > kMatteExtractMaxIds) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "matte_extract: id_count must be in 1..64");
    const float4* l[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int j = 0; j < ranks / 2; j++) {
        if (!layers[j]) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "matte_extract: layers[" + std::to_string(j) + "] is NULL");
        l[j] = (const float4*)layers[j];
    }
    MatteExtractIds set;
    for (int q = 0; q < kMatteExtractMaxIds; q++) set.id[q] = q < id_count ? matte_fix(ids[q]) : 0u;
    ENTER(ctx);
    launch_matte_extract(l, ranks, width * height, set, id_count, (float*)mask, ctx->stream);
    HIPOK(hipGetLastError());
    return PT_OK;
}

}  // extern "C"
