// common.h -- shared host-side helpers for the libvfmreg_hip.so translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vfmreg.h"
#include "config.h"

#define VFM_EXPORT extern "C" __attribute__((visibility("default")))

// thread-local last-error string (the only global state of the library)
char *vfm_err_buf();
int vfm_fail(int code, const char *fmt, ...);

#define VFM_CHECK_ARG(cond, ...)                                  \
    do {                                                          \
        if (!(cond)) return vfm_fail(VFM_EINVAL, __VA_ARGS__);    \
    } while (0)

#define VFM_CHECK_LAUNCH(what)                                                             \
    do {                                                                                   \
        hipError_t e__ = hipGetLastError();                                                \
        if (e__ != hipSuccess) return vfm_fail(VFM_EHIP, "%s: %s", what, hipGetErrorString(e__)); \
    } while (0)

#define VFM_CHECK_HIP(call)                                                                  \
    do {                                                                                     \
        hipError_t e__ = (call);                                                             \
        if (e__ != hipSuccess) return vfm_fail(VFM_EHIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

// pass a helper's failure on (the helper has already set the error text)
#define VFM_TRY(call)                    \
    do {                                 \
        const int rc__ = (call);         \
        if (rc__ != VFM_OK) return rc__; \
    } while (0)

// compute units of device `dev` / of the current device, asked for once per device (256 where the runtime cannot say)
static inline int vfm_compute_units_of(int dev) {
    static std::atomic<int> cus[64];
    int n = cus[dev & 63].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev & 63].store(n, std::memory_order_relaxed);
    }
    return n;
}
static inline int vfm_compute_units() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return vfm_compute_units_of(dev);
}

// hipFuncSetAttribute is per device: remember which devices have been configured (one bit each)
inline bool attr_done(unsigned long long mask) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return (mask >> (dev & 63)) & 1ull;
}
inline void attr_mark(unsigned long long& mask) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    mask |= 1ull << (dev & 63);
}
// ... and the whole of it for a kernel that may be launched from several host threads at once: `bytes` of dynamic LDS allowed to `kernel`
// on device `dev` (the current one), once per device on the kernel's own atomic mask
static inline int vfm_allow_dynamic_lds(const void* kernel, int bytes, int dev, std::atomic<unsigned long long>& done) {
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_relaxed) & bit) return VFM_OK;
    VFM_CHECK_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.fetch_or(bit, std::memory_order_relaxed);
    return VFM_OK;
}

static inline size_t vfm_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// carve consecutive 256-byte aligned regions out of a caller-provided workspace
struct VfmCarver {
    unsigned char *base;
    size_t off;
    explicit VfmCarver(void *p) : base(static_cast<unsigned char *>(p)), off(0) {}
    template <typename T>
    T *take(size_t count) {
        off = vfm_align_up(off, 256);
        T *r = reinterpret_cast<T *>(base ? base + off : nullptr);
        off += count * sizeof(T);
        return r;
    }
    size_t used() const { return vfm_align_up(off, 256); }
};
