// dev_buf_check.cpp -- csrc/dev_buf.h on the host alone: DevBuf and TempBuf over a counting malloc (stub/hip/hip_runtime.h), through grow,
// no-op, failed grow then grow, failed synchronise and the destruction of empty and full buffers.  Every allocation must be freed exactly
// once and nothing may dangle; tests/test_dev_buf_host.py builds this with -fsanitize=address,undefined and runs it.  No GPU, no library.
#include "dev_buf.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

static std::set<void*> live;              // what hipMalloc gave out and hipFree has not taken back
static int mallocs = 0, frees = 0, syncs = 0, double_frees = 0;
static bool fail_next_malloc = false, fail_next_sync = false;
static hipError_t last_error = hipSuccess;

hipError_t hipMalloc(void** ptr, size_t bytes) {
    if (fail_next_malloc) { fail_next_malloc = false; *ptr = (void*)0x1;  /* a failed call may leave anything here */ return last_error = hipErrorOutOfMemory; }
    *ptr = malloc(bytes ? bytes : 1);
    memset(*ptr, 0xab, bytes);
    live.insert(*ptr);
    mallocs++;
    return hipSuccess;
}
hipError_t hipFree(void* ptr) {
    if (!ptr) return hipSuccess;
    if (!live.erase(ptr)) { double_frees++; return last_error = hipErrorUnknown; }
    free(ptr);
    frees++;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
    syncs++;
    if (fail_next_sync) { fail_next_sync = false; return last_error = hipErrorUnknown; }
    return hipSuccess;
}
hipError_t hipGetLastError() { const hipError_t e = last_error; last_error = hipSuccess; return e; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "unknown error"; }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "dev_buf_check: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    using pt::DevBuf;
    using pt::TempBuf;
    hipStream_t stream = nullptr;
    {
        DevBuf empty;                                                   // destroyed without ever holding anything
        DevBuf b;
        CHECK(b.ptr == nullptr && b.cap == 0);
        // grow: synchronise first, then the caller's capacity, not the need
        CHECK(b.reserve(stream, 100, 158) == hipSuccess && b.cap == 158 && b.ptr && syncs == 1 && mallocs == 1 && frees == 0);
        memset(b.as<char>(), 1, 158);
        void* first = b.ptr;
        // no-op: no call at all
        CHECK(b.reserve(stream, 158, 1000) == hipSuccess && b.ptr == first && b.cap == 158 && syncs == 1 && mallocs == 1);
        // failed grow: the old array is gone, the buffer empty, the error left for the caller to clear
        fail_next_malloc = true;
        CHECK(b.reserve(stream, 159, 300) == hipErrorOutOfMemory && b.ptr == nullptr && b.cap == 0 && frees == 1 && live.empty());
        CHECK(hipGetLastError() == hipErrorOutOfMemory && hipGetLastError() == hipSuccess);
        // ... and the next grow succeeds from the empty state
        CHECK(b.reserve(stream, 159, 300) == hipSuccess && b.cap == 300 && mallocs == 2 && frees == 1);
        memset(b.as<char>(), 2, 300);
        // a failed synchronise: kernels may still read the array, so it stays
        void* second = b.ptr;
        fail_next_sync = true;
        CHECK(b.realloc(stream, 50) == hipErrorUnknown && b.ptr == second && b.cap == 300 && mallocs == 2 && frees == 1);
        // realloc to a smaller size (pt_denoise does that)
        CHECK(b.realloc(stream, 50) == hipSuccess && b.cap == 50 && mallocs == 3 && frees == 2 && live.size() == 1);
        // a buffer that failed and is destroyed empty
        DevBuf c;
        fail_next_malloc = true;
        CHECK(c.realloc(stream, 10) == hipErrorOutOfMemory && c.ptr == nullptr && c.cap == 0);
        // the temporaries of one call: no synchronise
        const int syncs_before = syncs;
        TempBuf t, u, never;
        CHECK(t.alloc(64) == hipSuccess && t.cap == 64 && t.as<int>() != nullptr);
        fail_next_malloc = true;
        CHECK(u.alloc(64) == hipErrorOutOfMemory && u.ptr == nullptr && u.cap == 0 && syncs == syncs_before);
        CHECK(live.size() == 2);
    }                                                                   // b (full), c, t (full), u, never, empty go
    CHECK(live.empty() && double_frees == 0 && mallocs == 4 && frees == 4);
    printf("dev_buf_check: %d allocations, %d frees, %d synchronises, nothing live\n", mallocs, frees, syncs);
    return 0;
}
