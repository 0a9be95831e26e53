// Mutation fuzzer of the accumulation checkpoint validator (gltf_renderer_amd/csrc/host/accum_state.cpp), built by
// tests/test_checkpoint_host.py with -fsanitize=address,undefined from that one file and this one.
//
//   accum_fuzz <seed dir> <iterations> <rng seed>
//
// Every *.acc file of the directory is a valid blob (written by tests/checkpoint_ref.py).  Each iteration copies one into a heap block
// of exactly its (possibly changed) length -- so that a read past the end is an AddressSanitizer report --, mutates it, and hands it to
// validate().  For every blob validate() accepts, each section is read through from the offsets the returned info implies, which must
// all lie inside the blob.  Half of the mutations re-seal the crc, so that the checks behind it are reached as well.
#include <dirent.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../gltf_renderer_amd/csrc/host/accum_state.h"

using namespace pt;

static uint64_t rng_state = 1;
static uint64_t rnd() {                         // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

// Reads every byte of every section at the offsets the info implies; returns false if one of them does not fit the blob.
static bool walk(const uint8_t* blob, size_t bytes, const pt_accum_info& info, uint64_t& sum) {
    const uint64_t P = (uint64_t)info.tiles * 256 * 16;
    uint64_t at = 160;
    auto section = [&](uint64_t n) {
        if (at > bytes || n > bytes - at) return false;
        for (uint64_t i = 0; i < n; i++) sum += blob[at + i];
        at += n;
        return true;
    };
    for (int k = 0; k < 3; k++)
        if ((info.sections & (1u << k)) && !section(P)) return false;
    if (info.sections & PT_ACCUM_ADAPTIVE) {
        const uint64_t rec = at;
        if (!section((uint64_t)info.tiles * 16)) return false;
        for (uint32_t t = 0; t < info.tiles; t++) {
            uint32_t w[4];
            memcpy(w, blob + rec + (uint64_t)t * 16, 16);
            if (w[0] > 1u || w[1] > (uint32_t)info.accumulated_frames || w[3] != 0u) return false;
        }
        if (!section(P)) return false;
    }
    const accum::Layout l = accum::layout(info.sections, info.tiles);
    return at == bytes && at == info.total_bytes && l.total_bytes == at;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: accum_fuzz <seed dir> <iterations> <rng seed>\n"); return 2; }
    const std::string dir = argv[1];
    const long iterations = atol(argv[2]);
    rng_state = strtoull(argv[3], nullptr, 10) * 2654435761ull + 1;
    std::vector<std::vector<uint8_t>> seeds;
    if (DIR* d = opendir(dir.c_str())) {
        while (dirent* e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() < 4 || n.substr(n.size() - 4) != ".acc") continue;
            FILE* f = fopen((dir + "/" + n).c_str(), "rb");
            if (!f) continue;
            std::vector<uint8_t> b;
            uint8_t buf[4096];
            size_t got;
            while ((got = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + got);
            fclose(f);
            seeds.push_back(b);
        }
        closedir(d);
    }
    if (seeds.empty()) { fprintf(stderr, "no seeds in %s\n", dir.c_str()); return 2; }

    // the seeds themselves must pass, and walk
    uint64_t sum = 0;
    for (const auto& s : seeds) {
        pt_accum_info info;
        std::string err;
        uint8_t* p = (uint8_t*)malloc(s.size());
        memcpy(p, s.data(), s.size());
        const bool ok = accum::validate(p, s.size(), info, nullptr, err) && walk(p, s.size(), info, sum);
        free(p);
        if (!ok) { fprintf(stderr, "a seed is refused: %s\n", err.c_str()); return 1; }
    }

    long accepted = 0, rejected = 0;
    for (long it = 0; it < iterations; it++) {
        const std::vector<uint8_t>& s = seeds[below(seeds.size())];
        size_t n = s.size();
        const uint64_t kind = below(8);
        if (kind == 0) n = below(s.size() + 1);                               // truncated anywhere
        else if (kind == 1) n = below(161);                                   // ... or inside the header
        else if (kind == 2) n = s.size() + 1 + below(64);                     // grown
        uint8_t* p = (uint8_t*)malloc(n ? n : 1);
        memcpy(p, s.data(), n < s.size() ? n : s.size());
        if (n > s.size()) memset(p + s.size(), (int)below(256), n - s.size());
        bool reseal = (rnd() & 1) != 0;
        if (n >= 160) {
            const int edits = 1 + (int)below(3);
            for (int e = 0; e < edits; e++) {
                const uint64_t how = below(6);
                if (how == 0) p[below(n)] ^= (uint8_t)(1u << below(8));                        // a bit anywhere
                else if (how == 1) p[below(160)] ^= (uint8_t)(1u << below(8));                 // a bit of the header
                else if (how == 2) p[below(160)] = (uint8_t)below(256);                        // a byte of the header
                else if (how == 3) {                                                           // a header word set to an edge value
                    static const uint32_t edge[] = {0u, 1u, 2u, 15u, 16u, 17u, 0x7fffffffu, 0x80000000u, 0xffffffffu, 1u << 30, (1u << 30) + 1u, 160u};
                    const uint32_t v = edge[below(sizeof(edge) / sizeof(edge[0]))];
                    memcpy(p + 4 * below(40), &v, 4);
                } else if (how == 4 && n > 160) p[160 + below(n - 160)] = (uint8_t)below(256); // a byte of the payload
                else if (how == 5) {                                                           // total_bytes follows the block's length
                    const uint64_t t = n;
                    memcpy(p + 16, &t, 8);
                }
            }
            if (reseal && n > 28) accum::seal(p, n);
        }
        pt_accum_info info;
        memset(&info, 0xa5, sizeof(info));
        std::string err;
        if (accum::validate(p, n, info, nullptr, err)) {
            accepted++;
            if (!walk(p, n, info, sum)) { fprintf(stderr, "an accepted blob does not hold its sections (iteration %ld)\n", it); free(p); return 1; }
        } else {
            rejected++;
            if (err.empty()) { fprintf(stderr, "a refusal without a message (iteration %ld)\n", it); free(p); return 1; }
        }
        free(p);
    }
    printf("fuzz: %ld iterations over %zu seeds, %ld accepted, %ld refused (checksum %llu)\n", iterations, seeds.size(), accepted, rejected,
           (unsigned long long)sum);
    return 0;
}
