// owned.h - the owners of the library's GPU resources: device memory, pinned host memory, streams, events and the small
// integer table made of the three.  Each is move-only, empty until its first reserve() / create(), empty again after a
// refused one, and gives back what it holds in its destructor; an empty owner's destructor makes no HIP call.  These are
// the only places of the library that call hipFree, hipHostFree, hipStreamDestroy and hipEventDestroy (conv3d.hip's two
// process-wide tables aside).  Host code only: no kernel and no __device__ function lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstring>

// One hipMalloc block.  A refused allocation reads HIP's sticky last-error state away, so that the next entry point's
// hipGetLastError() after a good launch does not report it.  Sites that cut one block into several regions take them at
// byte offsets: as<T>(offset).
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { free(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { free(); }
    void free() {
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
    }
    // at least `need` bytes: grow-only, and growing frees first - the contents are not kept
    hipError_t reserve(size_t need) {
        if (p && bytes >= need) return hipSuccess;
        free();
        const hipError_t r = hipMalloc(&p, need ? need : 16);
        if (r != hipSuccess) { p = nullptr; (void)hipGetLastError(); return r; }
        bytes = need;
        return hipSuccess;
    }
    bool alloc(size_t n, hipError_t *why = nullptr) {                // *why: what hipMalloc answered
        const hipError_t r = reserve(n);
        if (why) *why = r;
        return r == hipSuccess;
    }
    template <class T> T *as(size_t byte_offset = 0) const { return (T *)((char *)p + byte_offset); }
};

// The same for hipHostMalloc: pinned host memory (flags = hipHostMallocMapped: visible to kernels)
struct PinnedBuf {
    void *p = nullptr;
    size_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept {
        if (this != &o) { free(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~PinnedBuf() { free(); }
    void free() {
        if (p) (void)hipHostFree(p);
        p = nullptr; bytes = 0;
    }
    hipError_t reserve(size_t need, unsigned flags = hipHostMallocDefault) {
        if (p && bytes >= need) return hipSuccess;
        free();
        const hipError_t r = hipHostMalloc(&p, need, flags);
        if (r != hipSuccess) { p = nullptr; (void)hipGetLastError(); return r; }
        bytes = need;
        return hipSuccess;
    }
    template <class T> T *as() const { return (T *)p; }
};

// A non-blocking stream, made by the first create()
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream &operator=(Stream &&o) noexcept {
        if (this != &o) { reset(); s = o.s; o.s = nullptr; }
        return *this;
    }
    ~Stream() { reset(); }
    void reset() {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    }
    hipError_t create() {
        if (s) return hipSuccess;
        const hipError_t r = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (r != hipSuccess) { s = nullptr; (void)hipGetLastError(); }
        return r;
    }
    operator hipStream_t() const { return s; }
};

// An event, made by the first create(): for ordering (no timing) unless the flags say otherwise - hipEventDefault for
// the pairs that measure
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : ev(o.ev) { o.ev = nullptr; }
    Event &operator=(Event &&o) noexcept {
        if (this != &o) { reset(); ev = o.ev; o.ev = nullptr; }
        return *this;
    }
    ~Event() { reset(); }
    void reset() {
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
    }
    hipError_t create(unsigned flags = hipEventDisableTiming) {
        if (ev) return hipSuccess;
        const hipError_t r = hipEventCreateWithFlags(&ev, flags);
        if (r != hipSuccess) { ev = nullptr; (void)hipGetLastError(); }
        return r;
    }
    operator hipEvent_t() const { return ev; }
};

// A small integer table (patch origins, tile starts, a sharded caller's slot table) -> device without a stream
// synchronisation: the host copy lives in a pinned buffer of the table's; the only wait is for the PREVIOUS upload from
// that buffer to have been read (an event that has long fired by the next call).
struct IntTable {
    DevBuf dev;
    PinnedBuf host;
    Event read;                                                      // the previous upload from `host` has been read
    hipError_t upload(const int *src, size_t n, hipStream_t st) {
        const size_t bytes = n * sizeof(int) + 64;
        hipError_t r = dev.reserve(bytes);
        if (r == hipSuccess) r = read ? hipEventSynchronize(read) : read.create();
        if (r == hipSuccess) r = host.reserve(bytes);
        if (r != hipSuccess) return r;
        memcpy(host.p, src, n * sizeof(int));
        r = hipMemcpyAsync(dev.p, host.p, n * sizeof(int), hipMemcpyHostToDevice, st);
        return r == hipSuccess ? hipEventRecord(read, st) : r;
    }
    const int *data() const { return dev.as<int>(); }
};
