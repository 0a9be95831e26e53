// The node step's ray-space plane arithmetic against the candidate gate's own-box arithmetic, both compiled from csrc/pt_slab.h for the
// host (tests/test_slab_host.py builds this with -ffp-contract=off and runs it).  Checks, plane by plane,
//     the triangle's own box passes  =>  the node test passes:   slab_near(q) <= own_box_t(bound)  and  slab_far(q) >= own_box_t(bound)
// for every bound the builder may put behind the plane q (exactly P* = p + q s <= lo, or >= hi, and inside the node's box), and that the
// same planes WITHOUT the pad break it.  Then wide_write's loops (accel.hip), restated below over the same predicates, on bounds where the
// float plane equals the bound and the exact plane is past it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "pt_slab.h"

using namespace pt;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }
static double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }                 // [0, 1)
static double uni(double a, double b) { return a + (b - a) * uni(); }
static uint32_t pick(uint32_t n) { return (uint32_t)(rnd() % n); }

// the smallest float >= x / the largest float <= x, x a double
static float float_at_or_above(double x) { float f = (float)x; return (double)f >= x ? f : std::nextafterf(f, INFINITY); }
static float float_at_or_below(double x) { float f = (float)x; return (double)f <= x ? f : std::nextafterf(f, -INFINITY); }

struct Tally { uint64_t planes = 0, wrong = 0, dropped = 0, dropped_in_range = 0; double pad_used = 0; };

// One plane.  below: the plane is at or below the bound (a lo plane), else at or above it (a hi plane).
static void check_plane(Tally& t, bool pad, float step, float p, uint32_t q, float o, float inv, float bound, bool below) {
    SlabAxis ax = slab_axis(step, p, o, inv);
    const float E = 0.5f * (ax.Af - ax.An);
    if (!pad) { PT_NO_CONTRACT const float A = (p - o) * inv; ax.An = ax.Af = A; }
    const bool is_near = below == (inv > 0.0f);                 // a lo plane is met first by a ray that runs towards plus
    const float node = is_near ? slab_near((float)q, ax) : slab_far((float)q, ax);
    const float own = own_box_t(bound, o, inv);
    t.planes++;
    if (node != node) {                                       // fmaxf / fminf drop it: the plane is not tested
        t.dropped++;
        if (std::fabs(((double)p - (double)o) * (double)inv) < 1e38 && std::fabs((double)step * (double)inv) < 1e38 / 255) t.dropped_in_range++;
        return;
    }
    const bool ok = is_near ? node <= own : node >= own;
    if (!ok) {
        if (pad && t.wrong < 5) std::printf("  wrong side: step %a p %a q %u o %a inv %a bound %a: node %a own %a\n", step, p, q, o, inv, bound, node, own);
        t.wrong++;
    } else if (pad && std::isfinite(E) && E > 0 && std::isfinite(own) && std::isfinite(node)) {
        const double used = 1.0 - std::fabs((double)own - (double)node) / (double)E;      // the share of the pad that rounding consumed
        if (used > t.pad_used) t.pad_used = used;
    }
}

static void run_planes(Tally& t, bool pad, uint64_t n) {
    const uint32_t exps[] = {107u, 140u};                      // steps 2^-20 and 2^13
    const float inv_fixed[] = {1.0f, -1.0f, 1.0e30f, -1.0e30f};
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t e = pick(4) < 2 ? exps[pick(2)] : 90u + pick(60);
        const float step = bvh_step(e);
        // the node origin: a few thousand steps from zero up to 2^22 steps (a small node far from the coordinate origin), either sign, or zero
        float p = (float)(uni(-1, 1) * (double)step * std::pow(2.0, uni(0, 22)));
        if (pick(16) == 0) p = 0.0f;
        const uint32_t q = pick(4) == 0 ? 0u : (pick(3) == 0 ? 255u : pick(256));
        const double P = (double)p + (double)q * (double)step, top = (double)p + 255.0 * (double)step;      // exact (|p| / step < 2^45)
        float inv = pick(3) == 0 ? inv_fixed[pick(4)] : (float)((pick(2) ? 1.0 : -1.0) * std::pow(10.0, uni(0, 30)));
        float o;
        switch (pick(6)) {
            case 0: o = (float)P; break;                                                     // on the plane (exactly, where P is a float)
            case 1: o = p; break;                                                            // at the node origin: A = 0
            case 2: o = (float)((double)p + uni(0, 255) * (double)step); break;              // inside the node
            case 3: o = (float)((double)p + uni(-3000, 3000) * (double)step); break;         // outside, near
            case 4: o = (float)((double)p + uni(-1, 1) * 255e6 * (double)step); break;       // far outside: |A| >> 255 |S|
            default: o = (float)(P + uni(-2, 2) * (double)step * 1e-3); break;               // a hair off the plane
        }
        for (int below = 0; below < 2; below++) {
            // bounds the builder may leave behind this plane: the nearest float on the admitted side, its neighbour, one anywhere in the node
            float b[3];
            if (below) { b[0] = float_at_or_above(P); b[1] = std::nextafterf(b[0], INFINITY); b[2] = float_at_or_above(uni(P, top)); }
            else       { b[0] = float_at_or_below(P); b[1] = std::nextafterf(b[0], -INFINITY); b[2] = float_at_or_below(uni((double)p, P)); }
            for (int k = 0; k < 3; k++) {
                if ((double)b[k] < (double)p || (double)b[k] > top) continue;                // the node's box holds every bound under it
                check_plane(t, pad, step, p, q, o, inv, b[k], below != 0);
            }
        }
    }
}

// wide_write's search for one lo / hi byte (accel.hip), `exact`: with the check against the exact plane
static int quantise_lo(float lo, float p, uint32_t e, bool exact) {
    const float step = bvh_step(e), inv_step = bvh_step(254u - e);
    int ql = (int)std::floor((lo - p) * inv_step);
    ql = ql < 0 ? 0 : (ql > 255 ? 255 : ql);
    while (ql > 0 && (bvh_dequant((uint32_t)ql, step, p) > lo || (exact && bvh_plane_exceeds((uint32_t)ql, step, p, lo)))) ql--;
    return ql;
}
static int quantise_hi(float hi, float p, uint32_t e, bool exact) {
    const float step = bvh_step(e), inv_step = bvh_step(254u - e);
    int qh = (int)std::ceil((hi - p) * inv_step);
    qh = qh < 0 ? 0 : (qh > 255 ? 255 : qh);
    while (qh < 255 && (bvh_dequant((uint32_t)qh, step, p) < hi || (exact && bvh_plane_short_of((uint32_t)qh, step, p, hi)))) qh++;
    return qh;
}

static int run_builder() {
    int fail = 0;
    // the worked example: origin 2^-10 + 2^-33, step 2^-8, bound 2^-10 + 200 * 2^-8: fl(p + 200 s) is the bound, the exact plane is 2^-33 above it (and the mirror image for a hi).
    {
        const float p = 0x1p-10f + 0x1p-33f, lo = 0x1p-10f + 200 * 0x1p-8f; const uint32_t e = 127 - 8;
        const int qf = quantise_lo(lo, p, e, false), qx = quantise_lo(lo, p, e, true);
        const bool premise = bvh_dequant(200u, bvh_step(e), p) == lo && (double)p + 200.0 * 0x1p-8 > (double)lo;
        std::printf("worked lo example: float check alone %d, with the exact check %d, premise %d\n", qf, qx, (int)premise);
        if (!(premise && qf == 200 && qx == 199)) fail++;
        const float p2 = 0x1p-10f - 0x1p-34f, hi = 0x1p-10f + 200 * 0x1p-8f;
        const int hf = quantise_hi(hi, p2, e, false), hx = quantise_hi(hi, p2, e, true);
        const bool premise2 = bvh_dequant(200u, bvh_step(e), p2) == hi && (double)p2 + 200.0 * 0x1p-8 < (double)hi;
        std::printf("worked hi example: float check alone %d, with the exact check %d, premise %d\n", hf, hx, (int)premise2);
        if (!(premise2 && hf == 200 && hx == 201)) fail++;
    }
    // random nodes: origins with bits below the bounds' ulp
    uint64_t n = 0, float_only_wrong = 0, exact_wrong = 0, moved = 0;
    for (int i = 0; i < 2000000; i++) {
        const uint32_t e = 100u + pick(40);
        const double step = (double)bvh_step(e);
        const float p = (float)(uni(-1, 1) * step * std::pow(2.0, uni(-12, 12)));
        const float lo = float_at_or_above((double)p + uni(0, 255) * step), hi = float_at_or_below((double)p + uni(0, 255) * step);
        if ((double)lo > (double)p + 255 * step || (double)hi < (double)p) continue;
        const int qlf = quantise_lo(lo, p, e, false), qlx = quantise_lo(lo, p, e, true), qhf = quantise_hi(hi, p, e, false), qhx = quantise_hi(hi, p, e, true);
        n += 2;
        if ((double)p + qlf * step > (double)lo) float_only_wrong++;
        if ((double)p + qhf * step < (double)hi) float_only_wrong++;
        if ((double)p + qlx * step > (double)lo || bvh_dequant((uint32_t)qlx, bvh_step(e), p) > lo) exact_wrong++;
        if ((double)p + qhx * step < (double)hi || bvh_dequant((uint32_t)qhx, bvh_step(e), p) < hi) exact_wrong++;
        if (qlx != qlf || qhx != qhf) moved++;
        if (qlx > qlf || qhx < qhf || qlf - qlx > 1 || qhx - qhf > 1) exact_wrong++;                  // the exact check only ever loosens, by one
    }
    std::printf("builder: %llu bounds, exact plane past the bound with the float check alone %llu, with the exact check %llu, bytes moved %llu\n",
                (unsigned long long)n, (unsigned long long)float_only_wrong, (unsigned long long)exact_wrong, (unsigned long long)moved);
    if (float_only_wrong == 0 || exact_wrong != 0) fail++;
    return fail;
}

int main(int argc, char** argv) {
    const uint64_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 2500000ull;
    Tally with, without;
    run_planes(with, true, n);
    g_state = 0x9e3779b97f4a7c15ull;
    run_planes(without, false, n);
    std::printf("with the pad: %llu planes, wrong side %llu, dropped as NaN %llu (in range %llu), largest share of the pad used %.3f\n", (unsigned long long)with.planes,
                (unsigned long long)with.wrong, (unsigned long long)with.dropped, (unsigned long long)with.dropped_in_range, with.pad_used);
    std::printf("without the pad: %llu planes, wrong side %llu\n", (unsigned long long)without.planes, (unsigned long long)without.wrong);
    int fail = run_builder();
    if (with.wrong != 0 || with.dropped_in_range != 0 || without.wrong == 0) fail++;
    std::printf(fail ? "FAILED\n" : "ok\n");
    return fail ? 1 : 0;
}
