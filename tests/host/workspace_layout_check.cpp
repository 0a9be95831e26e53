// workspace_layout_check.cpp -- csrc/pt_workspace.h on the host alone, against the formulas it replaced.  The specification below restates
// them as they stood before the header existed: wavefront_workspace_bytes with its three bools, the three *_records_offset functions that
// called it back, and carve()'s walk over the arrays.  Over a grid of tiles, samples, stage workgroups and record combinations every offset
// and every total of the header must equal the specification's, every array must start on a 256-byte boundary, no two may overlap and the
// last must end inside the total.  tests/test_workspace_layout_host.py builds this with -fsanitize=address,undefined and runs it.
// No GPU, no library.
#include "pt_workspace.h"

#include <algorithm>
#include <cstdio>
#include <vector>

namespace spec {      // the formulas as they were; the constants are restated too, so that a changed constant in the header shows

constexpr uint32_t kShards = 256, kXcds = 8, kCounterStride = 16;
constexpr int kCounterArrays = 7, kBlock = 256;

uint32_t blocks_per_shard_for(int stage_blocks) {
    uint32_t b = (uint32_t)(stage_blocks > 0 ? stage_blocks : 1536) / kShards;
    return b < 1 ? 1 : b;
}
uint32_t gen_rounds_for(uint32_t my_tiles, uint32_t spp, uint32_t blocks_per_shard) {
    const uint32_t per_xcd = kShards * blocks_per_shard / kXcds;
    const uint32_t pairs = (my_tiles + kXcds - 1) / kXcds * spp;
    return (pairs + per_xcd - 1) / per_xcd;
}
uint32_t seg_cap_for(uint32_t my_tiles, uint32_t spp, uint32_t blocks_per_shard) { return gen_rounds_for(my_tiles, spp, blocks_per_shard) * blocks_per_shard * kBlock; }
uint32_t chunks_per_shard_for(size_t slots) { return (uint32_t)(((slots + kBlock - 1) / kBlock + kShards - 1) / kShards); }
size_t state_slots_for(size_t slots) { return (size_t)chunks_per_shard_for(slots) * kShards * kBlock; }

size_t workspace_bytes(uint32_t my_tiles, uint32_t spp, int stage_blocks, bool aov = false, bool matte = false, bool motion = false);
size_t aov_records_offset(uint32_t t, uint32_t spp, int sb) { return (workspace_bytes(t, spp, sb, false) + 255) & ~(size_t)255; }
size_t matte_records_offset(uint32_t t, uint32_t spp, int sb) { return (workspace_bytes(t, spp, sb, true) + 255) & ~(size_t)255; }
size_t motion_records_offset(uint32_t t, uint32_t spp, int sb) { return (workspace_bytes(t, spp, sb, true, true) + 255) & ~(size_t)255; }
size_t workspace_bytes(uint32_t my_tiles, uint32_t spp, int stage_blocks, bool aov, bool matte, bool motion) {
    const uint32_t bps = blocks_per_shard_for(stage_blocks);
    const size_t slots = state_slots_for((size_t)my_tiles * kBlock * spp);
    if (motion) return motion_records_offset(my_tiles, spp, stage_blocks) + slots * 16;
    if (matte) return matte_records_offset(my_tiles, spp, stage_blocks) + slots * 4;
    if (aov) return aov_records_offset(my_tiles, spp, stage_blocks) + slots * (2 * 16);
    const size_t q = (size_t)kShards * seg_cap_for(my_tiles, spp, bps);
    return slots * (5 * 16) + q * (4 * 16 + 4 * 16 + 16 + 2 * 16 + 2 * 2 * 16) + kCounterArrays * kShards * kCounterStride * 4 + 52 * 256;
}

// carve(): the offsets it handed out, in its order, with each array's bytes
struct Array { const char* name; size_t at, bytes; };
struct Carved {
    uint32_t blocks_per_shard, gen_rounds, seg_cap, chunks_per_shard;
    std::vector<Array> arrays;
};
Carved carve(uint32_t my_tiles, uint32_t spp, int stage_blocks) {
    const uint32_t slots = my_tiles * kBlock * spp;
    const size_t state_slots = state_slots_for(slots);
    Carved c;
    c.chunks_per_shard = chunks_per_shard_for(slots);
    size_t p = 0;
    auto take = [&](const char* name, size_t bytes) { c.arrays.push_back({name, p, bytes}); p += (bytes + 255) & ~(size_t)255; };
    c.blocks_per_shard = blocks_per_shard_for(stage_blocks);
    c.seg_cap = seg_cap_for(my_tiles, spp, c.blocks_per_shard);
    c.gen_rounds = gen_rounds_for(my_tiles, spp, c.blocks_per_shard);
    const size_t q = (size_t)kShards * c.seg_cap;
    for (int k = 0; k < kCounterArrays; k++) take("cnt", (size_t)kShards * kCounterStride * 4);
    take("L", state_slots * 16);
    take("beta_pdf", state_slots * 16);
    take("thr_misc", state_slots * 16);
    take("pend", state_slots * 32);
    for (int k = 0; k < 2; k++) { take("ray_o", q * 16); take("ray_d", q * 16); }
    for (int k = 0; k < 2; k++) { take("q_beta", q * 16); take("q_thr", q * 16); }
    take("hit", q * 16);
    take("env_a", q * 16);
    take("env_b", q * 16);
    take("sh_o", q * 2 * 16);
    take("sh_d", q * 2 * 16);
    return c;
}

}  // namespace spec

static long long cells = 0, failures = 0;
#define CHECK(cond) do { if (!(cond)) { if (failures++ < 20) fprintf(stderr, "workspace_layout_check: line %d: %s  (my_tiles %u, spp %u, stage_blocks %d, records %d%d%d)\n", \
                                                                     __LINE__, #cond, t, spp, sb, (int)aov, (int)matte, (int)motion); } } while (0)

static void check_cell(uint32_t t, uint32_t spp, int sb, bool aov, bool matte, bool motion) {
    cells++;
    const pt::WorkspaceLayout l = pt::workspace_layout(t, spp, sb, pt::WorkspaceRecords{aov, matte, motion}, 256);
    const spec::Carved c = spec::carve(t, spp, sb);
    // the figures carve() put into WfBuffers, and the helpers others call
    CHECK(l.blocks_per_shard == c.blocks_per_shard && l.gen_rounds == c.gen_rounds && l.seg_cap == c.seg_cap && l.chunks_per_shard == c.chunks_per_shard);
    CHECK(l.state_slots == spec::state_slots_for((size_t)t * 256 * spp));
    CHECK(pt::blocks_per_shard_for(sb) == spec::blocks_per_shard_for(sb));
    CHECK(pt::state_slots_for((size_t)t + 1, 256) == spec::state_slots_for((size_t)t + 1));             // (debug_trace_queues: slots that are no multiple of a tile)
    // every offset equal to the walk's, member by member in the walk's order
    const size_t mine[] = {l.cnt[0], l.cnt[1], l.cnt[2], l.cnt[3], l.cnt[4], l.cnt[5], l.cnt[6], l.L, l.beta_pdf, l.thr_misc, l.pend,
                           l.ray_o[0], l.ray_d[0], l.ray_o[1], l.ray_d[1], l.q_beta[0], l.q_thr[0], l.q_beta[1], l.q_thr[1],
                           l.hit, l.env_a, l.env_b, l.sh_o, l.sh_d};
    CHECK(sizeof(mine) / sizeof(mine[0]) == c.arrays.size());
    std::vector<spec::Array> all = c.arrays;
    for (size_t k = 0; k < all.size(); k++) { CHECK(mine[k] == all[k].at); all[k].at = mine[k]; }      // (below: the header's own offsets)
    for (int k = 1; k < pt::kCounterArrays; k++) CHECK(l.cnt[k] == l.cnt[0] + (size_t)k * pt::kShards * pt::kCounterStride * 4);     // one memset clears them
    // the record arrays: at the old offsets whether or not the earlier ones are in use
    const size_t s = l.state_slots;
    CHECK(l.rec_albedo == spec::aov_records_offset(t, spp, sb));
    CHECK(l.rec_normal == spec::aov_records_offset(t, spp, sb) + s * 16);                               // (launch_wavefront: rec_albedo + state_slots float4)
    CHECK(l.rec_matte == spec::matte_records_offset(t, spp, sb));
    CHECK(l.rec_motion == spec::motion_records_offset(t, spp, sb));
    CHECK(l.total == spec::workspace_bytes(t, spp, sb, aov, matte, motion));
    if (aov) { all.push_back({"rec_albedo", l.rec_albedo, s * 16}); all.push_back({"rec_normal", l.rec_normal, s * 16}); }
    if (matte) all.push_back({"rec_matte", l.rec_matte, s * 4});
    if (motion) all.push_back({"rec_motion", l.rec_motion, s * 16});
    // aligned, disjoint, inside the total
    std::sort(all.begin(), all.end(), [](const spec::Array& a, const spec::Array& b) { return a.at != b.at ? a.at < b.at : a.bytes < b.bytes; });
    for (size_t k = 0; k < all.size(); k++) {
        CHECK(all[k].at % 256 == 0);
        if (k + 1 < all.size()) CHECK(all[k].at + all[k].bytes <= all[k + 1].at);
        CHECK(all[k].at + all[k].bytes <= l.total);
    }
    // the tail pad stands between the carved arrays and the records
    const spec::Array& last = c.arrays.back();
    CHECK(l.rec_albedo == last.at + last.bytes + pt::kWorkspaceTailPad);
}

int main() {
    const uint32_t tiles[] = {0, 1, 2, 7, 8, 9, 255, 256, 257, 8160};           // 8160: 1920 x 1080
    const uint32_t spps[] = {1, 2, 3, 8, 64};
    const int stage[] = {0, 1, 255, 256, 512, 768, 1536};
    static_assert(pt::kShards == spec::kShards && pt::kXcds == spec::kXcds && pt::kCounterStride == spec::kCounterStride && pt::kCounterArrays == spec::kCounterArrays,
                  "the constants are the old ones");
    for (uint32_t t : tiles)
        for (uint32_t spp : spps)
            for (int sb : stage)
                for (int r = 0; r < 8; r++) check_cell(t, spp, sb, (r & 1) != 0, (r & 2) != 0, (r & 4) != 0);
    if (failures) { fprintf(stderr, "workspace_layout_check: %lld failed checks\n", failures); return 1; }
    printf("workspace_layout_check: %lld cells, every offset and total as before\n", cells);
    return 0;
}
