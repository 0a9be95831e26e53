// accum_state.h -- the accumulation checkpoint blob of pt_accum_save / pt_accum_load / pt_accum_inspect (include/mipt.h holds the
// format, field by field).  Plain C++, no HIP: the header, the crc, the validator and the header writer, so that a host program can
// link accum_state.cpp alone (tests/fuzz/accum_fuzz.cpp does).
#ifndef MIPT_ACCUM_STATE_H
#define MIPT_ACCUM_STATE_H

#include <cstddef>
#include <cstdint>
#include <string>

#include "mipt.h"

namespace pt {
namespace accum {

constexpr uint32_t kVersion = 1;
constexpr uint32_t kHeaderBytes = 160;
constexpr uint32_t kCrcFrom = 28;               // the crc covers bytes [28, total_bytes)
constexpr uint32_t kAllSections = PT_ACCUM_OUTPUT | PT_ACCUM_ALBEDO | PT_ACCUM_NORMAL_DEPTH | PT_ACCUM_ADAPTIVE;
constexpr uint32_t kMaxExtent = 1u << 30;
constexpr uint64_t kTileBytes = 256 * 16;       // one packed 16x16 tile of float4
constexpr uint64_t kRecordBytes = 16;           // one tile record {u32 active, u32 samples, f32 error, u32 0}

// The 160 bytes at the head of a blob.  Every field sits at its natural alignment, so the struct has no padding; it is copied in and
// out of a blob with memcpy (a blob may sit at any address).
struct Header {
    char     magic[8];                          //   0  "MIPTACC1"
    uint32_t version;                           //   8
    uint32_t header_bytes;                      //  12
    uint64_t total_bytes;                       //  16
    uint32_t crc32;                             //  24
    uint32_t sections;                          //  28
    uint32_t width, height;                     //  32, 36
    uint32_t tile_rank, tile_rank_count;        //  40, 44
    int32_t  accumulated_frames;                //  48
    uint32_t tiles;                             //  52
    uint64_t next_frame;                        //  56
    float    previous_world_to_clip[16];        //  64
    pt_adaptive_config adaptive;                // 128
    uint32_t reserved[4];                       // 144
};
static_assert(sizeof(Header) == kHeaderBytes, "the checkpoint header is 160 bytes");
static_assert(sizeof(pt_adaptive_config) == 16, "pt_adaptive_config is 16 bytes in the checkpoint header");

// Where the sections of a blob sit, from the fields of its info alone (64-bit throughout).  image[k] = 0 for an absent image.
struct Layout {
    uint64_t packed_bytes;                      // P: one image of the rank's tiles, tiles * 4096
    uint64_t image[3];                          // OUTPUT, ALBEDO, NORMAL_DEPTH
    uint64_t records, half;                     // ADAPTIVE: the tile records and the packed half buffer (0 without it)
    uint64_t total_bytes;
};

// IEEE 802.3 crc (the polynomial of zlib.crc32), continued from `crc` (0 to start).
uint32_t crc32(const void* data, size_t bytes, uint32_t crc = 0);

// Tiles (16x16, row-major) of rank `rank` among `world`: those with t % world == rank.
uint64_t tiles_of_rank(uint32_t width, uint32_t height, uint32_t rank, uint32_t world);

Layout layout(uint32_t sections, uint64_t tiles);

// Everything pt_accum_inspect promises.  On success fills `info` (and `previous_world_to_clip`, 16 floats, unless null); on failure `err`
// names the field and neither output is touched.
bool validate(const void* blob, size_t bytes, pt_accum_info& info, float* previous_world_to_clip, std::string& err);

// Writes the 160 header bytes for `info` (total_bytes and tiles are taken from it as given) with a zero crc; seal() then stores the
// crc of bytes [28, total_bytes) once the payload is in place.
void write_header(void* blob, const pt_accum_info& info, const float* previous_world_to_clip);
void seal(void* blob, uint64_t total_bytes);

}  // namespace accum
}  // namespace pt

#endif
