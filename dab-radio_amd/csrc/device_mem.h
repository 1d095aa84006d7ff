// device_mem.h -- the owners of what the host half takes from the runtime: device memory, pinned host memory, events, streams.
// A struct member of one of these types OWNS its handle and releases it when the struct is deleted; a raw pointer member only POINTS
// (into an owner's allocation, or at something another object owns).  Kernel argument lists and views take the raw handle from get().
// Nothing here waits: whoever frees memory the device may still use (a destroy function, a buffer that grows) waits first, at the site,
// for what that site knows to be in flight.  Includes nothing else of the library, so that the owners can be tested
// against a stand-in for the runtime (tests/cpp/device_mem_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <type_traits>

int dabgpu_check_hip(hipError_t e, const char* what);
void dabgpu_set_error(const char* fmt, ...);

namespace dabgpu {

// the untyped core of the two buffer owners: a block of device or pinned host memory and its capacity in bytes
class MemBlock {
    void* p_ = nullptr;
    size_t cap_ = 0;
    bool pinned_;
protected:
    explicit MemBlock(bool pinned) : pinned_(pinned) {}
    MemBlock(MemBlock&& o) noexcept : p_(o.p_), cap_(o.cap_), pinned_(o.pinned_) { o.p_ = nullptr; o.cap_ = 0; }
    MemBlock& operator=(MemBlock&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; } return *this; }
    ~MemBlock() { reset(); }
    void* ptr() const { return p_; }
    size_t cap_bytes() const { return cap_; }
    int alloc_bytes(size_t bytes, const char* what) {
        reset();
        const int st = dabgpu_check_hip(pinned_ ? hipHostMalloc(&p_, bytes, hipHostMallocDefault) : hipMalloc(&p_, bytes), what);
        if (st) p_ = nullptr; else cap_ = bytes;
        return st;
    }
public:
    MemBlock(const MemBlock&) = delete; MemBlock& operator=(const MemBlock&) = delete;
    void reset() { if (p_) (void)(pinned_ ? hipHostFree(p_) : hipFree(p_)); p_ = nullptr; cap_ = 0; }
    explicit operator bool() const { return p_ != nullptr; }
};

// the typed layer.  n: elements of T, bytes where T is void.  what = the label of a failure ("hipMalloc(stream bank)")
template <class T>
class MemBuffer : public MemBlock {
    static constexpr size_t UNIT = sizeof(typename std::conditional<std::is_void<T>::value, char, T>::type);
protected:
    using MemBlock::MemBlock;
public:
    T* get() const { return static_cast<T*>(ptr()); }
    size_t capacity() const { return cap_bytes() / UNIT; }
    // releases what was held, then allocates; empty (capacity 0) after a failure
    int alloc(size_t n, const char* what) { return alloc_bytes(n * UNIT, what); }
    // the grow-only step, once: `if (b.needs(n)) { the site's wait; st = b.regrow(n, what); }`
    bool needs(size_t n) const { return cap_bytes() < n * UNIT; }
    int regrow(size_t n, const char* what) { return needs(n) ? alloc(n, what) : 0; }
};
template <class T = void> struct DeviceBuffer : MemBuffer<T> { DeviceBuffer() : MemBuffer<T>(false) {} };      // hipMalloc / hipFree
template <class T = void> struct PinnedBuffer : MemBuffer<T> { PinnedBuffer() : MemBuffer<T>(true) {} };       // hipHostMalloc(hipHostMallocDefault) / hipHostFree

class Event {
    hipEvent_t e_ = nullptr;
public:
    Event() = default;
    Event(const Event&) = delete; Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
    ~Event() { reset(); }
    hipEvent_t get() const { return e_; }
    explicit operator bool() const { return e_ != nullptr; }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    // flags: hipEventDisableTiming, or dabgpu_wait_event_flags(...) for an event a host thread waits on
    int create(unsigned flags, const char* what) {
        reset();
        const int st = dabgpu_check_hip(hipEventCreateWithFlags(&e_, flags), what);
        if (st) e_ = nullptr;                // (whatever a failed call left there)
        return st;
    }
};

class Stream {
    hipStream_t s_ = nullptr;
    int made(hipError_t e, const char* what) { const int st = dabgpu_check_hip(e, what); if (st) s_ = nullptr; return st; }
public:
    Stream() = default;
    Stream(const Stream&) = delete; Stream& operator=(const Stream&) = delete;
    Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; } return *this; }
    ~Stream() { reset(); }
    hipStream_t get() const { return s_; }
    explicit operator bool() const { return s_ != nullptr; }
    void reset() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
    int create(unsigned flags, const char* what) { reset(); return made(hipStreamCreateWithFlags(&s_, flags), what); }
    int create(unsigned flags, int priority, const char* what) { reset(); return made(hipStreamCreateWithPriority(&s_, flags, priority), what); }
};

}  // namespace dabgpu
