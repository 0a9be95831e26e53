// accum_state.cpp -- see accum_state.h.  No HIP, no allocation beyond the error string: validate() reads `bytes` bytes and nothing else.
#include "accum_state.h"

#include <cmath>
#include <cstring>

namespace pt {
namespace accum {

namespace {

const char kMagic[8] = {'M', 'I', 'P', 'T', 'A', 'C', 'C', '1'};

struct CrcTable {
    uint32_t t[8][256];
    CrcTable() {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; i++)
            for (int s = 1; s < 8; s++) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xffu];
    }
};

bool fail(std::string& err, const char* what) {
    err = std::string("accumulation blob: ") + what;
    return false;
}

}  // namespace

uint32_t crc32(const void* data, size_t bytes, uint32_t crc) {
    static const CrcTable table;
    const uint8_t* p = (const uint8_t*)data;
    uint32_t c = ~crc;
    while (bytes >= 8) {                        // eight bytes a step (slicing by 8), read byte by byte: no alignment or endianness assumed
        const uint32_t lo = c ^ ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
        c = table.t[7][lo & 0xffu] ^ table.t[6][(lo >> 8) & 0xffu] ^ table.t[5][(lo >> 16) & 0xffu] ^ table.t[4][lo >> 24] ^
            table.t[3][p[4]] ^ table.t[2][p[5]] ^ table.t[1][p[6]] ^ table.t[0][p[7]];
        p += 8; bytes -= 8;
    }
    while (bytes--) c = table.t[0][(c ^ *p++) & 0xffu] ^ (c >> 8);
    return ~c;
}

uint64_t tiles_of_rank(uint32_t width, uint32_t height, uint32_t rank, uint32_t world) {
    if (world == 0 || rank >= world) return 0;
    const uint64_t n = (uint64_t)((width + (uint64_t)PT_TILE - 1) / PT_TILE) * ((height + (uint64_t)PT_TILE - 1) / PT_TILE);
    return n > rank ? (n - rank + world - 1) / world : 0;
}

Layout layout(uint32_t sections, uint64_t tiles) {
    Layout l;
    memset(&l, 0, sizeof(l));
    l.packed_bytes = tiles * kTileBytes;
    uint64_t at = kHeaderBytes;
    for (int k = 0; k < 3; k++)
        if (sections & (1u << k)) { l.image[k] = at; at += l.packed_bytes; }
    if (sections & PT_ACCUM_ADAPTIVE) {
        l.records = at; at += tiles * kRecordBytes;
        l.half = at; at += l.packed_bytes;
    }
    l.total_bytes = at;
    return l;
}

bool validate(const void* blob, size_t bytes, pt_accum_info& info, float* previous_world_to_clip, std::string& err) {
    if (!blob) return fail(err, "null");
    if (bytes < kHeaderBytes) return fail(err, "shorter than its 160-byte header");
    Header h;
    memcpy(&h, blob, sizeof(h));
    if (memcmp(h.magic, kMagic, 8) != 0) return fail(err, "magic");
    if (h.version != kVersion) return fail(err, "version");
    if (h.header_bytes != kHeaderBytes) return fail(err, "header_bytes");
    if (h.total_bytes != (uint64_t)bytes) return fail(err, "total_bytes differs from the size given");
    if (h.sections & ~kAllSections) return fail(err, "sections: unknown bit");
    if (!(h.sections & PT_ACCUM_OUTPUT)) return fail(err, "sections: no output image");
    for (uint32_t r : h.reserved)
        if (r != 0) return fail(err, "reserved words");
    if (h.width == 0 || h.width > kMaxExtent) return fail(err, "width");
    if (h.height == 0 || h.height > kMaxExtent) return fail(err, "height");
    if (h.tile_rank_count == 0) return fail(err, "tile_rank_count");
    if (h.tile_rank >= h.tile_rank_count) return fail(err, "tile_rank");
    if ((uint64_t)h.tiles != tiles_of_rank(h.width, h.height, h.tile_rank, h.tile_rank_count)) return fail(err, "tiles");
    if (h.accumulated_frames < 1) return fail(err, "accumulated_frames");
    const Layout l = layout(h.sections, h.tiles);
    if (h.total_bytes != l.total_bytes) return fail(err, "total_bytes differs from what the sections need");
    if (h.sections & PT_ACCUM_ADAPTIVE) {       // what pt_set_adaptive accepts, and enabled: the section exists for an enabled config only
        const pt_adaptive_config& a = h.adaptive;
        if (a.enable == 0) return fail(err, "adaptive.enable");
        if (a.min_samples < 2) return fail(err, "adaptive.min_samples");
        if (a.max_samples < a.min_samples) return fail(err, "adaptive.max_samples");
        if (!std::isfinite(a.threshold) || a.threshold < 0.0f) return fail(err, "adaptive.threshold");
    } else {
        const uint8_t zero[sizeof(pt_adaptive_config)] = {0};
        if (memcmp(&h.adaptive, zero, sizeof(zero)) != 0) return fail(err, "adaptive config without the adaptive section");
    }
    if (crc32((const uint8_t*)blob + kCrcFrom, bytes - kCrcFrom) != h.crc32) return fail(err, "crc32");
    if (h.sections & PT_ACCUM_ADAPTIVE) {
        const uint8_t* rec = (const uint8_t*)blob + l.records;
        for (uint64_t t = 0; t < h.tiles; t++, rec += kRecordBytes) {
            uint32_t w[4];
            float e;
            memcpy(w, rec, 16);
            memcpy(&e, rec + 8, 4);
            if (w[0] > 1u) return fail(err, "tile record: active");
            if (w[1] > (uint32_t)h.accumulated_frames) return fail(err, "tile record: samples beyond accumulated_frames");
            if (w[0] == 1u && w[1] != (uint32_t)h.accumulated_frames) return fail(err, "tile record: an active tile short of accumulated_frames");
            if (e != e) return fail(err, "tile record: error is NaN");
            if (w[3] != 0u) return fail(err, "tile record: pad");
        }
    }
    info.sections = h.sections;
    info.width = h.width; info.height = h.height;
    info.tile_rank = h.tile_rank; info.tile_rank_count = h.tile_rank_count;
    info.accumulated_frames = h.accumulated_frames;
    info.tiles = h.tiles;
    info.next_frame = h.next_frame;
    info.total_bytes = h.total_bytes;
    info.adaptive = h.adaptive;
    if (previous_world_to_clip) memcpy(previous_world_to_clip, h.previous_world_to_clip, 64);
    return true;
}

void write_header(void* blob, const pt_accum_info& info, const float* previous_world_to_clip) {
    Header h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, kMagic, 8);
    h.version = kVersion;
    h.header_bytes = kHeaderBytes;
    h.total_bytes = info.total_bytes;
    h.sections = info.sections;
    h.width = info.width; h.height = info.height;
    h.tile_rank = info.tile_rank; h.tile_rank_count = info.tile_rank_count;
    h.accumulated_frames = info.accumulated_frames;
    h.tiles = info.tiles;
    h.next_frame = info.next_frame;
    memcpy(h.previous_world_to_clip, previous_world_to_clip, 64);
    if (info.sections & PT_ACCUM_ADAPTIVE) h.adaptive = info.adaptive;
    memcpy(blob, &h, sizeof(h));
}

void seal(void* blob, uint64_t total_bytes) {
    const uint32_t c = crc32((const uint8_t*)blob + kCrcFrom, (size_t)(total_bytes - kCrcFrom));
    memcpy((uint8_t*)blob + 24, &c, 4);
}

}  // namespace accum
}  // namespace pt
