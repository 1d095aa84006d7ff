// A stand-in for <hip/hip_runtime.h>, for tests/cpp/device_mem_host.cpp ONLY (never on the library's include path): the calls
// csrc/device_mem.h makes, over malloc / free, with a counter per call, a "fail the Nth allocation" switch and a log of releases.
// Every release is checked: what is handed back must be live and of the kind it is handed back as, or the program aborts.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <vector>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct stub_event* hipEvent_t;
typedef struct stub_stream* hipStream_t;
enum { hipHostMallocDefault = 0, hipEventDisableTiming = 2, hipEventBlockingSync = 1, hipStreamNonBlocking = 1 };

namespace hip_stub {
enum Kind { DEVICE, PINNED, EVENT, STREAM, KINDS };
struct State {
    long made[KINDS] = {}, released[KINDS] = {};
    long calls = 0;                           // every runtime call
    long fail_at = 0, allocations = 0;        // fail_at = N > 0: the Nth allocation (of any kind) from now on fails
    std::map<void*, Kind> live;
    std::vector<void*> release_log;
};
inline State& state() { static State s; return s; }
inline hipError_t make(void** p, size_t bytes, Kind k) {
    State& s = state();
    s.calls++;
    if (s.fail_at > 0 && ++s.allocations == s.fail_at) { *p = reinterpret_cast<void*>(0x1);  /* garbage an owner must not keep */ return hipErrorOutOfMemory; }
    *p = malloc(bytes ? bytes : 1);
    s.live[*p] = k; s.made[k]++;
    return hipSuccess;
}
inline hipError_t release(void* p, Kind k) {
    State& s = state();
    s.calls++;
    auto it = s.live.find(p);
    if (it == s.live.end() || it->second != k) { fprintf(stderr, "hip_stub: release of %p, which is not live as kind %d\n", p, (int)k); abort(); }
    s.live.erase(it); s.released[k]++; s.release_log.push_back(p);
    free(p);
    return hipSuccess;
}
}  // namespace hip_stub

inline hipError_t hipMalloc(void** p, size_t bytes) { return hip_stub::make(p, bytes, hip_stub::DEVICE); }
inline hipError_t hipFree(void* p) { return hip_stub::release(p, hip_stub::DEVICE); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return hip_stub::make(p, bytes, hip_stub::PINNED); }
inline hipError_t hipHostFree(void* p) { return hip_stub::release(p, hip_stub::PINNED); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hip_stub::make(reinterpret_cast<void**>(e), 1, hip_stub::EVENT); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return hip_stub::release(e, hip_stub::EVENT); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return hip_stub::make(reinterpret_cast<void**>(s), 1, hip_stub::STREAM); }
inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return hip_stub::make(reinterpret_cast<void**>(s), 1, hip_stub::STREAM); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return hip_stub::release(s, hip_stub::STREAM); }
