// threads_check.cpp -- the threading model of the plain-C++ scene side, exercised: one thread per scene (include/mipt_scene.h: the scene
// is single-threaded, gs_last_error is per thread), every thread's FIRST use of the library concurrent with the others'.
// Test infrastructure: built twice by tests/test_threads_host.py (-fsanitize=thread and plain -O2) from this file, image_decode.cpp,
// gltf_scene.cpp and accum_state.cpp; CPU only, the device C-ABI the loader would call on upload is stubbed out.
//
//   threads_check <phase> <dir>        phase: png | images | gltf-datauri | glb | errors | accum
//
// One phase per process, so that each lazily built table's first use is the concurrent one: eight threads are released together by a
// barrier, nothing of the library is called before it, and after the join the main thread repeats every thread's work serially and
// compares byte for byte.  <dir> holds the seed files of tools/fuzz_host.py write_seeds plus dynamic.png; the phases write there.
// Exit 0 = pass; 1 = a difference or a refused call (named on stderr); 2 = usage / missing input.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mipt.h"
#include "../../include/mipt_scene.h"
#include "../../gltf_renderer_amd/csrc/host/accum_state.h"

// ---- stubs for the device-side C-ABI (never reached: nothing here uploads)
extern "C" {
int pt_buffer_create(pt_ctx*, const void*, size_t, int, int*) { return -1; }
int pt_texture_create(pt_ctx*, const uint8_t*, int, int, int, int*) { return -1; }
int pt_sampler_create(pt_ctx*, const pt_sampler_desc*, int*) { return -1; }
int pt_scene_set_materials(pt_ctx*, const pt_material*, int) { return -1; }
int pt_scene_set_lights(pt_ctx*, const pt_light*, int) { return -1; }
int pt_scene_set_instances(pt_ctx*, const pt_instance_desc*, int) { return -1; }
int pt_skin_run(pt_ctx*, const pt_skin_params*, const pt_bone*, int) { return -1; }
const char* pt_last_error(const pt_ctx*) { return "stub"; }
int pt_buffer_destroy(pt_ctx*, int) { return -1; }
int pt_texture_destroy(pt_ctx*, int) { return -1; }
}

namespace {

constexpr int kThreads = 8;
using Bytes = std::vector<uint8_t>;

std::string g_dir;                                   // set in main before any thread exists, read-only afterwards

bool read_file(const std::string& p, Bytes& d) {
    d.clear();
    FILE* f = fopen(p.c_str(), "rb");
    if (!f) return false;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + got);
    fclose(f);
    return true;
}
bool write_file(const std::string& p, const uint8_t* d, size_t n) {
    FILE* f = fopen(p.c_str(), "wb");
    if (!f) return false;
    const bool ok = n == 0 || fwrite(d, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

template <class T> void put(Bytes& out, const T& v) { const uint8_t* p = (const uint8_t*)&v; out.insert(out.end(), p, p + sizeof(T)); }
void put(Bytes& out, const void* p, size_t n) { if (p && n) out.insert(out.end(), (const uint8_t*)p, (const uint8_t*)p + n); }

struct Fnv {                                         // FNV-1a, 64 bit
    uint64_t h = 1469598103934665603ull;
    void add(const void* p, size_t n) { const uint8_t* b = (const uint8_t*)p; for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; } }
    template <class T> void pod(const T& v) { add(&v, sizeof(T)); }
    void stream(const void* p, size_t n) { const uint8_t present = p != nullptr; pod(present); if (p) add(p, n); }
};

// The barrier: every thread counts itself in and spins until all have.
std::atomic<int> g_arrived{0};
void barrier_wait() {
    g_arrived.fetch_add(1);
    while (g_arrived.load() < kThreads) std::this_thread::yield();
}

// work(t, result, err): thread t's deterministic piece of work; false = a call was refused or a result is wrong (err says what).
using Work = std::function<bool(int, Bytes&, std::string&)>;

// Eight threads through the barrier, then the same work serially on this thread; every thread's bytes must be the serial bytes, and,
// with `all_equal`, every thread's bytes the same.
int run(const char* phase, const Work& work, bool all_equal) {
    Bytes results[kThreads];
    std::string errs[kThreads];
    bool ok[kThreads] = {};
    std::vector<std::thread> threads;
    for (int t = 0; t < kThreads; t++)
        threads.emplace_back([&, t] { barrier_wait(); ok[t] = work(t, results[t], errs[t]); });
    for (auto& th : threads) th.join();
    int bad = 0;
    for (int t = 0; t < kThreads; t++)
        if (!ok[t]) { fprintf(stderr, "%s: thread %d: %s\n", phase, t, errs[t].c_str()); bad++; }
    for (int t = 0; t < kThreads; t++) {
        Bytes want;
        std::string err;
        if (!work(t, want, err)) { fprintf(stderr, "%s: serial repeat of thread %d: %s\n", phase, t, err.c_str()); bad++; continue; }
        if (want != results[t]) {
            size_t at = 0;
            while (at < want.size() && at < results[t].size() && want[at] == results[t][at]) at++;
            fprintf(stderr, "%s: thread %d differs from its serial repeat at byte %zu (%zu bytes threaded, %zu serial)\n", phase, t, at, results[t].size(), want.size());
            bad++;
        }
        if (all_equal && results[t] != results[0]) { fprintf(stderr, "%s: thread %d differs from thread 0\n", phase, t); bad++; }
    }
    if (!bad) printf("%s: %d threads, %zu result bytes each way, all equal\n", phase, kThreads, results[0].size());
    return bad ? 1 : 0;
}

std::string last_error() { const char* e = gs_last_error(); return e ? e : ""; }

// ---- 1. png: the writer's crc table, the decoder's fixed-Huffman tables (img_write_png deflates with the fixed code), then a dynamic one
bool png_work(int t, Bytes& out, std::string& err) {
    const int w = 33, h = 17;
    Bytes px((size_t)w * h * 4);
    uint32_t s = 12345u + 977u * (uint32_t)t;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int c = 0; c < 4; c++) {            // smooth ramps (matches for the LZ77 stage) with a little noise (literals)
                s = s * 1664525u + 1013904223u;
                px[((size_t)y * w + x) * 4 + c] = (uint8_t)(x * (3 + c) + y * (5 + t) + ((s >> 24) & 3));
            }
    const std::string path = g_dir + "/thread_" + std::to_string(t) + ".png";
    if (img_write_png(path.c_str(), px.data(), w, h, 4) != 0) { err = "img_write_png: " + last_error(); return false; }
    Bytes file;
    if (!read_file(path, file)) { err = "cannot read back " + path; return false; }
    int gw = 0, gh = 0;
    uint8_t* got = nullptr;
    if (img_load_rgba8(path.c_str(), &gw, &gh, &got) != 0 || !got) { err = "img_load_rgba8 of the file just written: " + last_error(); return false; }
    const bool same = gw == w && gh == h && memcmp(got, px.data(), px.size()) == 0;
    put(out, file.data(), file.size()); put(out, gw); put(out, gh); put(out, got, (size_t)gw * gh * 4);
    img_free(got);
    if (!same) { err = "the decoded image is not the image written"; return false; }
    Bytes dyn;
    if (!read_file(g_dir + "/dynamic.png", dyn)) { err = "dynamic.png is missing"; return false; }
    got = nullptr;
    if (img_decode_rgba8(dyn.data(), dyn.size(), &gw, &gh, &got) != 0 || !got) { err = "img_decode_rgba8(dynamic.png): " + last_error(); return false; }
    put(out, gw); put(out, gh); put(out, got, (size_t)gw * gh * 4);
    img_free(got);
    return true;
}

// ---- 2. images: every other decoder path
const char* const kImages[] = {"base.jpg", "prog.jpg", "grey.jpg", "rle.hdr", "flat.hdr", "c0_half.exr", "c0_float.exr", "c1_half.exr", "c1_float.exr",
                               "c2_half.exr", "c2_float.exr", "c3_half.exr", "c3_float.exr"};
constexpr int kNumImages = (int)(sizeof(kImages) / sizeof(kImages[0]));

bool images_work(int t, Bytes& out, std::string& err) {
    Bytes part[kNumImages];
    for (int k = 0; k < kNumImages; k++) {
        const int i = (k + t * 2) % kNumImages;      // every thread starts with another file
        const std::string name = kImages[i];
        Bytes d;
        if (!read_file(g_dir + "/" + name, d)) { err = name + " is missing"; return false; }
        int w = 0, h = 0, half = -1;
        if (name.size() > 4 && name.compare(name.size() - 4, 4, ".jpg") == 0) {
            uint8_t* px = nullptr;
            if (img_decode_rgba8(d.data(), d.size(), &w, &h, &px) != 0 || !px) { err = name + ": " + last_error(); return false; }
            put(part[i], w); put(part[i], h); put(part[i], px, (size_t)w * h * 4);
            img_free(px);
        } else {
            float* px = nullptr;
            const int is_exr = name.compare(name.size() - 4, 4, ".exr") == 0;
            if (img_decode_rgb32f(d.data(), d.size(), is_exr, &w, &h, &half, &px) != 0 || !px) { err = name + ": " + last_error(); return false; }
            put(part[i], w); put(part[i], h); put(part[i], half); put(part[i], px, (size_t)w * h * 3 * sizeof(float));
            img_free(px);
        }
    }
    for (int i = 0; i < kNumImages; i++) put(out, part[i].data(), part[i].size());
    return true;
}

// ---- 3, 4. a scene file: everything gs_get_* returns, then the posed hierarchy at four times, one 64-bit digest per category
#define GS(call) do { if ((call) < 0) { err = std::string(#call) + ": " + last_error(); gs_free(sc); return false; } } while (0)

bool scene_digests(const std::string& path, Bytes& out, std::string& err) {
    gs_scene* sc = nullptr;
    if (gs_load_file(path.c_str(), &sc) != 0 || !sc) { err = "gs_load_file: " + last_error(); return false; }
    gs_counts c;
    memset(&c, 0, sizeof(c));
    GS(gs_get_counts(sc, &c));
    Fnv counts, prims, morphs, materials, textures, samplers, cameras, nodes, skins, channels;
    counts.pod(c);
    for (int p = 0; p < c.primitives; p++) {
        gs_primitive_info pi;
        GS(gs_get_primitive(sc, p, &pi));
        const int head[] = {pi.mesh, pi.index_in_mesh, pi.flags, pi.topology, pi.num_vertices, pi.num_indices, pi.index_format, pi.material_id, pi.num_targets};
        prims.pod(head);
        const size_t nv = (size_t)pi.num_vertices;
        prims.stream(pi.index, (size_t)pi.num_indices * (pi.index_format == PT_FORMAT_R16_UINT ? 2 : 4));
        prims.stream(pi.position, nv * 12); prims.stream(pi.tangent_space, nv * 4);
        prims.stream(pi.texcoord[0], nv * 8); prims.stream(pi.texcoord[1], nv * 8);
        prims.stream(pi.color, nv * 8); prims.stream(pi.joint_weight, nv * 16);
        for (int k = 0; k < pi.num_targets; k++) {
            int flags = 0; const float* pos = nullptr; const uint32_t* ts = nullptr;
            GS(gs_get_morph_target(sc, p, k, &flags, &pos, &ts));
            morphs.pod(flags); morphs.stream(pos, nv * 12); morphs.stream(ts, nv * 4);
        }
    }
    for (int m = 0; m < c.materials; m++) { pt_material mat; memset(&mat, 0, sizeof(mat)); GS(gs_get_material(sc, m, &mat)); materials.pod(mat); }
    for (int i = 0; i < c.textures; i++) {
        int w = 0, h = 0, srgb = 0, loaded = 0; const uint8_t* px = nullptr;
        GS(gs_get_texture(sc, i, &w, &h, &srgb, &loaded, &px));
        const int head[] = {w, h, srgb, loaded};
        textures.pod(head); textures.stream(px, (size_t)w * h * 4);
    }
    for (int i = 0; i < c.samplers; i++) { pt_sampler_desc d; memset(&d, 0, sizeof(d)); GS(gs_get_sampler(sc, i, &d)); samplers.pod(d); }
    for (int i = 0; i < c.cameras; i++) { gs_camera_info ci; memset(&ci, 0, sizeof(ci)); GS(gs_get_camera(sc, i, &ci)); cameras.pod(ci); }
    auto pose = [&](Fnv& f) -> bool {                // every node, its weights and bones; the roots and lights of every scene
        for (int n = 0; n < c.nodes; n++) {
            gs_node_info ni; memset(&ni, 0, sizeof(ni));
            if (gs_get_node(sc, n, &ni) < 0) return false;
            f.pod(ni);
            float w[16] = {0};
            const int nw = gs_get_node_weights(sc, n, w, 16);
            if (nw < 0) return false;
            f.pod(nw); f.pod(w);
            std::vector<pt_bone> bones(64);
            memset(bones.data(), 0, bones.size() * sizeof(pt_bone));
            const int nb = gs_gather_bones(sc, n, bones.data(), 64);
            if (nb < 0) return false;
            f.pod(nb); f.add(bones.data(), (size_t)(nb < 64 ? nb : 64) * sizeof(pt_bone));
        }
        for (int s = 0; s < c.scenes; s++) {
            int roots[64] = {0};
            const int nr = gs_get_scene_nodes(sc, s, roots, 64);
            pt_light lights[16];
            memset(lights, 0, sizeof(lights));
            const int nl = gs_gather_lights(sc, s, lights, 16);
            if (nr < 0 || nl < 0) return false;
            f.pod(nr); f.pod(roots); f.pod(nl); f.add(lights, (size_t)(nl < 16 ? nl : 16) * sizeof(pt_light));
        }
        return true;
    };
    GS(gs_calculate_global_transforms(sc, 0));
    if (!pose(nodes)) { err = "rest pose: " + last_error(); gs_free(sc); return false; }
    for (int k = 0; k < c.skins; k++) {
        int nj = 0; const uint32_t* joints = nullptr; const float* ibp = nullptr;
        GS(gs_get_skin(sc, k, &nj, &joints, &ibp));
        skins.pod(nj); skins.stream(joints, (size_t)nj * 4); skins.stream(ibp, (size_t)nj * 64);
    }
    float length = 0;
    for (int a = 0; a < c.animations; a++) {
        int nch = 0;
        GS(gs_get_animation(sc, a, &length, &nch));
        channels.pod(length); channels.pod(nch);
        for (int ch = 0; ch < nch; ch++) {
            gs_channel_info ci;
            GS(gs_get_channel(sc, a, ch, &ci));
            const int head[] = {ci.node, ci.path, ci.interpolation, ci.format, ci.width, ci.num_times, ci.num_transform_bytes};
            channels.pod(head); channels.stream(ci.times, (size_t)ci.num_times * 4); channels.stream(ci.transforms, (size_t)ci.num_transform_bytes);
        }
    }
    for (const Fnv* f : {&counts, &prims, &morphs, &materials, &textures, &samplers, &cameras, &nodes, &skins, &channels}) put(out, f->h);
    const float times[4] = {0.0f, 0.37f * length, length, 2.0f * length + 1.0f};
    for (float time : times) {
        Fnv posed;
        if (c.animations > 0) GS(gs_animate(sc, c.animations - 1, time));
        GS(gs_calculate_global_transforms(sc, 0));
        if (!pose(posed)) { err = "posed hierarchy: " + last_error(); gs_free(sc); return false; }
        put(out, posed.h);
    }
    gs_free(sc);
    return true;
}

// ---- 5. errors: a thread's failures are its own (gs_last_error is thread_local), and do not disturb the threads that succeed
constexpr int kRounds = 50;
std::thread::id g_main;                              // set in main before any thread exists
bool fresh_thread_is(bool error_empty) { return error_empty || std::this_thread::get_id() == g_main; }
std::string trunc_path(int t) { return g_dir + "/trunc_" + std::to_string(t) + ".glb"; }

bool errors_work(int t, Bytes& out, std::string& err) {
    if (t & 1) {
        const std::string path = trunc_path(t);
        std::string first;
        for (int r = 0; r < kRounds; r++) {
            gs_scene* sc = (gs_scene*)(uintptr_t)1;
            const int rc = gs_load_file(path.c_str(), &sc);
            if (rc == 0 || sc != nullptr) { err = "a truncated file was loaded"; if (rc == 0) gs_free(sc); return false; }
            const std::string e = last_error();
            if (e.compare(0, path.size(), path) != 0) { err = "round " + std::to_string(r) + ": gs_last_error is not this thread's: \"" + e + "\""; return false; }
            if (r == 0) first = e;
            if (e != first) { err = "round " + std::to_string(r) + ": \"" + e + "\" after \"" + first + "\""; return false; }
        }
        put(out, first.data(), first.size());
        return true;
    }
    Bytes first;
    const std::string before = last_error();         // empty on a fresh thread; the serial repeat's thread has failures of its own behind it
    if (!fresh_thread_is(before.empty())) { err = "a thread that has called nothing reads the error \"" + before + "\""; return false; }
    for (int r = 0; r < kRounds; r++) {
        Bytes d;
        if (!scene_digests(g_dir + "/sink.glb", d, err)) return false;
        if (last_error() != before) { err = "round " + std::to_string(r) + ": a thread that never failed reads the error \"" + last_error() + "\""; return false; }
        if (r == 0) first = d;
        if (d != first) { err = "round " + std::to_string(r) + ": the digests changed"; return false; }
    }
    out = first;
    return true;
}

// ---- 6. accum: header, crc and validator on a blob per thread
bool accum_work(int t, Bytes& out, std::string& err) {
    using namespace pt;
    pt_accum_info info;
    memset(&info, 0, sizeof(info));
    info.sections = PT_ACCUM_OUTPUT | ((t & 1) ? PT_ACCUM_ALBEDO : 0) | ((t & 2) ? PT_ACCUM_NORMAL_DEPTH : 0) | ((t & 4) ? PT_ACCUM_ADAPTIVE : 0);
    info.width = 17 + 13 * (uint32_t)t; info.height = 9 + 7 * (uint32_t)t;
    info.tile_rank_count = 1 + (uint32_t)t % 3; info.tile_rank = (uint32_t)t % info.tile_rank_count;
    info.accumulated_frames = 3 + t;
    info.tiles = (uint32_t)accum::tiles_of_rank(info.width, info.height, info.tile_rank, info.tile_rank_count);
    info.next_frame = 1000u + (uint64_t)t;
    if (info.sections & PT_ACCUM_ADAPTIVE) info.adaptive = {1, 2, 64, 0.02f * (float)(t + 1)};
    const accum::Layout l = accum::layout(info.sections, info.tiles);
    info.total_bytes = l.total_bytes;
    Bytes blob((size_t)l.total_bytes);
    uint32_t s = 99u + 31u * (uint32_t)t;
    for (size_t i = accum::kHeaderBytes; i < blob.size(); i++) { s = s * 1664525u + 1013904223u; blob[i] = (uint8_t)(s >> 24); }
    if (info.sections & PT_ACCUM_ADAPTIVE)
        for (uint32_t k = 0; k < info.tiles; k++) {
            const uint32_t active = (k + (uint32_t)t) & 1u;
            const uint32_t rec[4] = {active, active ? (uint32_t)info.accumulated_frames : k % (uint32_t)(info.accumulated_frames + 1), 0, 0};
            const float e = 0.01f * (float)k;
            memcpy(&blob[(size_t)l.records + (size_t)k * 16], rec, 16);
            memcpy(&blob[(size_t)l.records + (size_t)k * 16 + 8], &e, 4);
        }
    float w2c[16];
    for (int i = 0; i < 16; i++) w2c[i] = (float)(i * (t + 1)) * 0.25f;
    accum::write_header(blob.data(), info, w2c);
    accum::seal(blob.data(), info.total_bytes);
    pt_accum_info got;
    memset(&got, 0, sizeof(got));
    float got_w2c[16] = {0};
    std::string verr;
    if (!accum::validate(blob.data(), blob.size(), got, got_w2c, verr)) { err = "the sealed blob is refused: " + verr; return false; }
    if (memcmp(&got, &info, sizeof(info)) != 0 || memcmp(got_w2c, w2c, sizeof(w2c)) != 0) { err = "validate returns another info than was written"; return false; }
    put(out, blob.data(), blob.size());
    blob[blob.size() - 1 - (size_t)t] ^= 0x10;       // a payload bit (of an image: never a tile record)
    if (accum::validate(blob.data(), blob.size(), got, nullptr, verr) || verr.find("crc32") == std::string::npos) { err = "a flipped payload bit is not a crc32 refusal: " + verr; return false; }
    put(out, verr.data(), verr.size());
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: threads_check png|images|gltf-datauri|glb|errors|accum <dir>\n"); return 2; }
    const std::string phase = argv[1];
    g_dir = argv[2];
    g_main = std::this_thread::get_id();
    if (phase == "png") return run("png", png_work, false);
    if (phase == "images") return run("images", images_work, true);
    if (phase == "gltf-datauri") return run("gltf-datauri", [](int, Bytes& o, std::string& e) { return scene_digests(g_dir + "/sink.gltf", o, e); }, true);
    if (phase == "glb") return run("glb", [](int, Bytes& o, std::string& e) { return scene_digests(g_dir + "/sink.glb", o, e); }, true);
    if (phase == "errors") {
        Bytes good;                                  // plain file I/O, nothing of the library: a truncated copy of its own for every failing thread
        if (!read_file(g_dir + "/sink.glb", good) || good.size() < 64) { fprintf(stderr, "errors: sink.glb is missing\n"); return 2; }
        for (int t = 1; t < kThreads; t += 2)
            if (!write_file(trunc_path(t), good.data(), good.size() * (size_t)(t + 1) / 10)) { fprintf(stderr, "errors: cannot write %s\n", trunc_path(t).c_str()); return 2; }
        return run("errors", errors_work, false);
    }
    if (phase == "accum") return run("accum", accum_work, false);
    fprintf(stderr, "unknown phase %s\n", phase.c_str());
    return 2;
}
