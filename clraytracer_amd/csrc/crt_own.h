// crt_own.h -- owners of what the host side allocates: device buffers, pinned host buffers, events, streams
// Part of the one translation unit crt_shim.hip (included there, in this order: crt_own.h, crt_state.h, crt_instances.h, crt_upload.h,
// crt_bvh_driver.h, crt_frame.h, crt_query_host.h, crt_ao_host.h, crt_multidev.h); everything here has internal linkage.
//
// Four move-only types, the only callers of the HIP create / destroy functions in this directory. What a session creates is a member
// of its State (or a local of the function that needs it) and is released exactly once, by the destructor: no list of things to free.
// The destructors call HIP, so an owner must die with its device current -- State dies in destroy_group only (crt_multidev.h), which
// selects the device first. No release(), no sharing: an alias (State::stream, the table pointers into instBlock) is a plain pointer
// that must not outlive the owner.
#pragma once
namespace {

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { return (int)e_; } } while (0)
#define RCCHK(x) do { int r_ = (x); if (r_ != CRT_OK) { return r_; } } while (0)

// Owned objects alive in this process (crt_debug_live_resources, which is its only reader): +1 per successful alloc / create, -1 per
// release. Atomic: the secondary devices of a session allocate from their worker threads.
std::atomic<long> gLiveOwned{0};

// A device allocation of `capacity()` elements of T.
template <class T> class DevBuf {
    T* p = nullptr; size_t cap = 0;
    void free() { if (p) { (void)hipFree(p); --gLiveOwned; } p = nullptr; cap = 0; }
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { free(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { free(); }
    // `count` elements, uninitialised; whatever was held before is freed first. On failure empty, capacity 0.
    int alloc(size_t count)
    {
        free();
        HIPCHK(hipMalloc(&p, count * sizeof(T)));
        cap = count; ++gLiveOwned;
        return CRT_OK;
    }
    // Room for `count` elements (no-op when there is): waits for `s`, the stream that last used the buffer, frees it and allocates
    // anew. Contents are not kept. On failure empty, capacity 0.
    int grow(size_t count, hipStream_t s)
    {
        if (count <= cap) return CRT_OK;
        HIPCHK(hipStreamSynchronize(s));
        return alloc(count);
    }
    size_t capacity() const { return cap; }
    operator T*() const { return p; }
};

// The same in pinned host memory (hipHostMalloc with `flags`). Growing replaces the block without waiting for anything: the caller
// knows that nothing queued still reads it.
template <class T> class PinnedBuf {
    T* p = nullptr; size_t cap = 0;
    void free() { if (p) { (void)hipHostFree(p); --gLiveOwned; } p = nullptr; cap = 0; }
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { free(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~PinnedBuf() { free(); }
    int alloc(size_t count, unsigned flags)
    {
        free();
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&p), count * sizeof(T), flags));
        cap = count; ++gLiveOwned;
        return CRT_OK;
    }
    int grow(size_t count, unsigned flags) { return count <= cap ? (int)CRT_OK : alloc(count, flags); }
    size_t capacity() const { return cap; }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};

// An event / a stream: create(flags) once, the destructor destroys.
class Event {
    hipEvent_t e = nullptr;
    void destroy() { if (e) { (void)hipEventDestroy(e); --gLiveOwned; } e = nullptr; }
public:
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { if (this != &o) { destroy(); e = o.e; o.e = nullptr; } return *this; }
    ~Event() { destroy(); }
    int create(unsigned flags = hipEventDefault)
    {
        destroy();
        HIPCHK(hipEventCreateWithFlags(&e, flags));
        ++gLiveOwned;
        return CRT_OK;
    }
    operator hipEvent_t() const { return e; }
};

class Stream {
    hipStream_t s = nullptr;
    void destroy() { if (s) { (void)hipStreamDestroy(s); --gLiveOwned; } s = nullptr; }
public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    Stream& operator=(Stream&& o) noexcept { if (this != &o) { destroy(); s = o.s; o.s = nullptr; } return *this; }
    ~Stream() { destroy(); }
    int create(unsigned flags)
    {
        destroy();
        HIPCHK(hipStreamCreateWithFlags(&s, flags));
        ++gLiveOwned;
        return CRT_OK;
    }
    operator hipStream_t() const { return s; }
};

} // namespace
