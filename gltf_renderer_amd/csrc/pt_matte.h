// pt_matte.h -- ID mattes (pt_set_matte, include/mipt.h): the exponent fix of an id and the fold of a pixel's ranked (id, coverage) pairs,
// shared by k_wf_matte_resolve (wf_passes.hip) and the host entry points and k_matte_extract (matte.hip).  tests/matte_ref.py restates it.
//
// Ids are 32-bit patterns that travel through float4 images: they are moved and compared as integers only (__float_as_uint /
// __uint_as_float are register renames), never through float arithmetic or a float compare -- an id may read as any normal float.
// A pixel's K ranks live in 2 K registers: every loop below runs over a template constant and is fully unrolled, every index is static.
#pragma once
#include "pt_math.h"

namespace pt {

// Cryptomatte's exponent fix: an id read as a float is finite and normal (and so never 0)
__host__ __device__ inline uint32_t matte_fix(uint32_t h) {
    const uint32_t e = (h >> 23) & 0xffu;
    return (e == 0u || e == 255u) ? h ^ (1u << 23) : h;
}

PT_DEV float4 blend_aov(float4 h, int accumulated, float4 v);           // pt_wf_stage.h: the running mean of four components

template <int R>
struct MatteRanks { uint32_t id[R]; float cov[R]; };                    // id 0 = an empty rank, whose coverage is +0

// Layer j of a pixel holds ranks 2j and 2j + 1: (id bits, coverage, id bits, coverage)
template <int R>
PT_DEV void matte_unpack(MatteRanks<R>& m, int j, const float4 v) {
    m.id[2 * j] = __float_as_uint(v.x); m.cov[2 * j] = v.y; m.id[2 * j + 1] = __float_as_uint(v.z); m.cov[2 * j + 1] = v.w;
}
template <int R>
PT_DEV float4 matte_pack(const MatteRanks<R>& m, int j) {
    return make_float4(__uint_as_float(m.id[2 * j]), m.cov[2 * j], __uint_as_float(m.id[2 * j + 1]), m.cov[2 * j + 1]);
}

// One sample with record h (0 = no hit) into a pixel that holds n samples.
template <int R>
PT_DEV void matte_fold_sample(MatteRanks<R>& m, uint32_t h, int n) {
    if (n == 0) {
#pragma unroll
        for (int r = 0; r < R; r++) { m.id[r] = 0u; m.cov[r] = 0.0f; }
        if (h != 0u) { m.id[0] = h; m.cov[0] = 1.0f; }
        return;
    }
    // every rank moves towards 1 if it holds the sample's id and towards 0 otherwise; an empty rank has c = x = 0 and stays +0
    bool held = false;
#pragma unroll
    for (int g = 0; g < R; g += 4) {
        float c[4], x[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool in = g + k < R, is = in && h != 0u && m.id[in ? g + k : 0] == h;
            c[k] = in ? m.cov[in ? g + k : 0] : 0.0f;
            x[k] = is ? 1.0f : 0.0f;
            held = held || is;
        }
        const float4 o = blend_aov(make_float4(c[0], c[1], c[2], c[3]), n, make_float4(x[0], x[1], x[2], x[3]));
        const float oc[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int k = 0; k < 4; k++) if (g + k < R) m.cov[g + k] = oc[k];
    }
    // a new id takes an empty rank with the weight of one sample; with no rank empty it is dropped
    bool place = h != 0u && !held;
    const float b = fdiv(1.0f, (float)n + 1.0f);
#pragma unroll
    for (int r = 0; r < R; r++) {
        const bool here = place && m.id[r] == 0u;
        m.id[r] = here ? h : m.id[r];
        m.cov[r] = here ? b : m.cov[r];
        place = place && !here;
    }
}

// The order of a pixel's ranks: non-empty before empty, then coverage descending, then id ascending as unsigned.  Total, so the sorted
// state depends only on the multiset of pairs.
PT_DEV bool matte_before(uint32_t ia, float ca, uint32_t ib, float cb) {
    const bool na = ia != 0u, nb = ib != 0u;
    if (na != nb) return na;
    if (ca != cb) return ca > cb;
    return ia < ib;
}
template <int R>
PT_DEV void matte_cx(MatteRanks<R>& m, int i, int j) {                  // compare-exchange: afterwards rank i is not behind rank j
    const bool swap = matte_before(m.id[j], m.cov[j], m.id[i], m.cov[i]);
    const uint32_t ii = m.id[i], ij = m.id[j];
    const float ci = m.cov[i], cj = m.cov[j];
    m.id[i] = swap ? ij : ii; m.id[j] = swap ? ii : ij;
    m.cov[i] = swap ? cj : ci; m.cov[j] = swap ? ci : cj;
}
// Sorting networks of minimal size for 2, 4, 6 and 8 inputs (1, 5, 12 and 19 comparators), on static indices
template <int R>
PT_DEV void matte_sort(MatteRanks<R>& m) {
    static_assert(R == 2 || R == 4 || R == 6 || R == 8, "ranks");
    if constexpr (R == 2) {
        matte_cx(m, 0, 1);
    } else if constexpr (R == 4) {
        matte_cx(m, 0, 1); matte_cx(m, 2, 3);
        matte_cx(m, 0, 2); matte_cx(m, 1, 3);
        matte_cx(m, 1, 2);
    } else if constexpr (R == 6) {
        matte_cx(m, 0, 5); matte_cx(m, 1, 3); matte_cx(m, 2, 4);
        matte_cx(m, 1, 2); matte_cx(m, 3, 4);
        matte_cx(m, 0, 3); matte_cx(m, 2, 5);
        matte_cx(m, 0, 1); matte_cx(m, 2, 3); matte_cx(m, 4, 5);
        matte_cx(m, 1, 2); matte_cx(m, 3, 4);
    } else {
        matte_cx(m, 0, 2); matte_cx(m, 1, 3); matte_cx(m, 4, 6); matte_cx(m, 5, 7);
        matte_cx(m, 0, 4); matte_cx(m, 1, 5); matte_cx(m, 2, 6); matte_cx(m, 3, 7);
        matte_cx(m, 0, 1); matte_cx(m, 2, 3); matte_cx(m, 4, 5); matte_cx(m, 6, 7);
        matte_cx(m, 2, 4); matte_cx(m, 3, 5);
        matte_cx(m, 1, 4); matte_cx(m, 3, 6);
        matte_cx(m, 1, 2); matte_cx(m, 3, 4); matte_cx(m, 5, 6);
    }
}

}  // namespace pt
