// liw_host_common.hpp — host scaffolding that the fleet C ABIs (liw_lfe_*, liw_floop_*, liw_fpg_*) share: the device probe of their
// create calls, the part of a handle the compute entries check, and the synchronous copies between a store and the host.  Host-only;
// everything is in an anonymous namespace, so no symbol of it reaches the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/liw_window.h"   // LIW_EINVAL, LIW_ENODEV

namespace {

inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// Is `device` a gfx950 device?  *err says why not, when a device is there to say it of; the probe's own HIP error is cleared.
inline bool liw_probe_gfx950(int device, std::string* err) {
    bool have = false;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev) {
        hipDeviceProp_t props;
        if (hipGetDeviceProperties(&props, device) == hipSuccess) {
            if (std::strstr(props.gcnArchName, "gfx950") != nullptr) have = true;
            else *err = std::string("device is ") + props.gcnArchName + ", this library is built for gfx950 only";
        }
    }
    (void)hipGetLastError();
    if (!have && err->empty()) *err = "no HIP device";
    return have;
}

struct liw_fleet_ctx_base {      // liw_lfe_ctx, liw_floop_ctx and liw_fpg_ctx derive from it
    int device = 0;
    bool have_device = false;
    std::string err;
};

inline int fail(liw_fleet_ctx_base* c, int code, const char* what) {
    if (c) c->err = what;
    return code;
}

// head of every compute entry: a handle, a device, and that device current
#define LIW_FLEET_DEV(c)                                                                                  \
    do {                                                                                                  \
        if (!(c)) return LIW_EINVAL;                                                                      \
        if (!(c)->have_device) return fail((c), LIW_ENODEV, "no usable gfx950 device (no CPU fallback)"); \
        (void)hipSetDevice((c)->device);                                                                  \
    } while (0)

inline bool bad_store(const void* store) { return !store || ((uintptr_t)store & 7) != 0; }

// synchronous copies of n elements at byte offset off of a store; nothing to copy is a success
template <class T> bool pull(const void* store, size_t off, T* dst, size_t n) {
    return n == 0 || hipMemcpy(dst, (const char*)store + off, sizeof(T) * n, hipMemcpyDeviceToHost) == hipSuccess;
}
template <class T> bool push(void* store, size_t off, const T* src, size_t n) {
    return n == 0 || hipMemcpy((char*)store + off, src, sizeof(T) * n, hipMemcpyHostToDevice) == hipSuccess;
}

}  // namespace
