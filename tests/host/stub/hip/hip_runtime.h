// Stand-in for <hip/hip_runtime.h> when csrc/dev_buf.h is compiled for the host alone (tests/host/dev_buf_check.cpp): the five runtime
// calls an owner of device memory can make, over malloc, counted.
#pragma once
#include <cstddef>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
typedef struct stub_stream* hipStream_t;

hipError_t hipMalloc(void** ptr, size_t bytes);
hipError_t hipFree(void* ptr);
hipError_t hipStreamSynchronize(hipStream_t stream);
hipError_t hipGetLastError();
const char* hipGetErrorString(hipError_t e);
