/* Internal: what the host sources of the library (*_host.cpp) share.  Not installed, nothing of it exported (exports.map). */
#ifndef MI_HOST_COMMON_H
#define MI_HOST_COMMON_H
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <new>

#include "../../include/mi_dmrecon.h"

/* dmrecon_host.cpp: the thread-local error message and the context's device */
int mi_host_fail(int code, const char* msg);
int mi_host_ctx_device(const mi_dmrecon_ctx* c);

/* What a module keeps per context: made by the module's first call on the context, deleted by mi_dmrecon_ctx_destroy with
 * the context's device current and its streams idle. */
struct HostModule { virtual ~HostModule() = default; };
enum { MI_MODULE_RANSAC, MI_MODULE_SIFT, MI_MODULE_SURF, MI_MODULE_BA, MI_MODULE_COUNT };
HostModule*& mi_host_ctx_module(mi_dmrecon_ctx* c, int which);

/* (not variadic on purpose: the call sites pass int32_t for %lld and rely on the conversion to long long) */
inline int failf(int code, const char* fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
    char buf[320];
    std::snprintf(buf, sizeof(buf), fmt, a, b, c, d);
    return mi_host_fail(code, buf);
}

#define MI_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            char _b[256];                                                                     \
            std::snprintf(_b, sizeof(_b), "%s failed: %s", #expr, hipGetErrorString(_e));     \
            return mi_host_fail(MI_DMRECON_EDEVICE, _b);                                      \
        }                                                                                     \
    } while (0)

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

/* device (or pinned host) memory that only grows, to exactly what was asked for; a failed need() leaves it empty */
struct Buf {
    void* p = nullptr;
    size_t cap = 0;
    bool host = false;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }
    hipError_t need(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        hipError_t e = host ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes; else p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)(host ? hipHostFree(p) : hipFree(p));
        p = nullptr; cap = 0;
    }
};
struct PinnedBuf : Buf { PinnedBuf() { host = true; } };

/* A C entry point's body: no exception crosses the C ABI */
template <class Body>
int guarded(Body body) {
    try { return body(); }
    catch (const std::bad_alloc&) { return mi_host_fail(MI_DMRECON_EDEVICE, "out of host memory"); }
}

#endif
