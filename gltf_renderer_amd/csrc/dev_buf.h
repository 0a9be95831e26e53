// dev_buf.h -- the one owner of a device allocation on the host side of libmipt.so (pt_ctx's scratch and tables, the hooks' temporaries).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace pt {

// A device array that is thrown away and allocated anew when it has to grow; what it held is not kept.  Freed with its owner: a pt_ctx is
// deleted by pt_destroy with its device current and its stream drained.
struct DevBuf {
    void* ptr = nullptr;
    size_t cap = 0;                  // bytes

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { hipFree(ptr); }
    template <typename T> T* as() const { return (T*)ptr; }

    // Kernels already enqueued on `stream` may still read the old array: drain it, free, allocate `bytes`.  A failed synchronise leaves the
    // buffer as it was; a failed allocation leaves it empty (its error stays for the caller's hipGetLastError to clear).
    hipError_t realloc(hipStream_t stream, size_t bytes) {
        hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return e;
        hipFree(ptr);
        ptr = nullptr; cap = 0;
        if ((e = hipMalloc(&ptr, bytes)) != hipSuccess) { ptr = nullptr; return e; }
        cap = bytes;
        return hipSuccess;
    }
    // Room for `need` bytes; a buffer that lacks it is reallocated with `new_cap` (the caller's slack rule).
    hipError_t reserve(hipStream_t stream, size_t need, size_t new_cap) { return need > cap ? realloc(stream, new_cap) : hipSuccess; }
};

// A temporary of one call: nothing enqueued can know it yet, so it is allocated without the synchronise, once, and freed at the end of the scope.
struct TempBuf : DevBuf {
    hipError_t alloc(size_t bytes) {
        const hipError_t e = hipMalloc(&ptr, bytes);
        if (e != hipSuccess) ptr = nullptr; else cap = bytes;
        return e;
    }
};

}  // namespace pt
