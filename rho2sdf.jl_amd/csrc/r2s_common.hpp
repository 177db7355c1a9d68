// Shared host-side helpers of the library (error string, HIP error check, device buffers).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>

#include "../../include/rho2sdf_hip.h"

inline thread_local std::string g_err;
inline int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(R2S_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                               \
    } while (0)

// bytes of device memory that live DevBufs hold (r2s_live_device_bytes); touched on growth and free only
inline std::atomic<int64_t> g_live_device_bytes{0};

// A device buffer.  It owns what it points to: it frees in its destructor (on whichever device is current when it dies)
// and moves by stealing the pointer.  An object of static storage duration must not hold one by value - the HIP runtime
// may be gone before a static destructor runs (see PerDevice in r2s_internal.hpp).
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p;
            cap = o.cap;
            o.p = nullptr;
            o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return 0;
        release();
        size_t want = bytes + bytes / 4 + 256;
        if (hipMalloc(&p, want) != hipSuccess) {
            (void)hipGetLastError();
            if (hipMalloc(&p, bytes) != hipSuccess) return -1;
            want = bytes;
        }
        cap = want;
        g_live_device_bytes += (int64_t)cap;
        return 0;
    }
    int ensure_exact(size_t bytes)   // no growth margin (very large buffers)
    {
        if (bytes <= cap) return 0;
        release();
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return -1;
        }
        cap = bytes;
        g_live_device_bytes += (int64_t)cap;
        return 0;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        g_live_device_bytes -= (int64_t)cap;
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() { return reinterpret_cast<T*>(p); }
    template <class T>
    const T* as() const { return reinterpret_cast<const T*>(p); }
};

// a pinned host block that frees itself
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { release(); }
    hipError_t ensure(size_t bytes, unsigned flags = hipHostMallocDefault)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        const hipError_t e = hipHostMalloc(&p, bytes, flags);
        if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return e; }
        cap = bytes;
        return hipSuccess;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// an event / a stream that destroys itself: created into .h, read as the plain handle
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
    Handle& operator=(Handle&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Handle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

inline int check_device(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(R2S_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
    }
    if (device >= n) return fail(R2S_ERR_ARG, "device %d out of range (%d devices)", device, n);
    return 0;
}

// resolve `device` (-1 = current) and make it current
inline int use_device(int device)
{
    int rc = check_device(device < 0 ? 0 : device);
    if (rc) return rc;
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    return 0;
}

#define ENSURE(buf, bytes)                                                       \
    do {                                                                         \
        if ((buf).ensure(bytes)) return fail(R2S_ERR_NOMEM, "hipMalloc of %zu bytes failed", (size_t)(bytes)); \
    } while (0)
