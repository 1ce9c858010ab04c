// host_call.h - the host side of one call of an entry point outside the engine (prep, resample, export_labels, postprocess,
// ensemble, ensemble_resample, metrics, imageio, reorient, deflate_masks, ops_api): owned scratch (DevBuf, owned.h), the status chain of one call on
// one stream, the refusals the entries share and the dispatch from a dtype code to an element type.  Host code only: no
// kernel and no __device__ function lives here.
#pragma once
#include "fnn_device.h"
#include "owned.h"
#include "../../include/fnn.h"
#include <cstdarg>
#include <cstdio>
#include <initializer_list>

int fnn_failf(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
inline int fnn_failf(int code, const char *fmt, ...) {
    char msg[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    return fnn_fail(code, msg);
}

// The HIP calls of one entry-point call on one stream: each runs only while nothing before it has failed, a launch is
// followed by hipGetLastError(), and finish() ends the call - synchronise, then FNN_OK or FNN_E_HIP with HIP's text.
struct HipCall {
    hipStream_t st;
    hipError_t r = hipSuccess;
    explicit HipCall(void *stream) : st((hipStream_t)stream) {}
    bool ok() const { return r == hipSuccess; }
    HipCall &copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
        if (ok()) r = hipMemcpyAsync(dst, src, bytes, kind, st);
        return *this;
    }
    HipCall &fill(void *dst, int byte, size_t bytes) {
        if (ok()) r = hipMemsetAsync(dst, byte, bytes, st);
        return *this;
    }
    template <class K, class... A> HipCall &launch(K kernel, dim3 grid, dim3 block, size_t lds, const A &...args) {
        if (ok()) {
            hipLaunchKernelGGL(kernel, grid, block, (unsigned)lds, st, args...);
            r = hipGetLastError();
        }
        return *this;
    }
    bool sync() {
        if (ok()) r = hipStreamSynchronize(st);
        return ok();
    }
    int fail() const { return fnn_fail(FNN_E_HIP, hipGetErrorString(r)); }
    int finish() { return sync() ? FNN_OK : fail(); }
};

// ---- the refusals the entries share: FNN_OK, or the code with the message set
inline bool fnn_is_perm(const int32_t t[3]) {
    int seen = 0;
    for (int i = 0; i < 3; ++i) if (t[i] >= 0 && t[i] <= 2) seen |= 1 << t[i];
    return seen == 7;
}
inline int fnn_check_perm(const int32_t t[3], const char *name) {
    return fnn_is_perm(t) ? FNN_OK : fnn_failf(FNN_E_INVALID, "%s is not a permutation of (0, 1, 2)", name);
}
inline int fnn_check_label_dtype(int d) {
    return d == FNN_LABEL_U8 || d == FNN_LABEL_U16 ? FNN_OK : fnn_fail(FNN_E_INVALID, "unknown label dtype");
}
inline int fnn_check_float_dtype(int d, const char *what = "dtype") {
    return d == FNN_OUT_F16 || d == FNN_OUT_F32 ? FNN_OK : fnn_failf(FNN_E_INVALID, "unknown %s", what);
}
// every pointer of the list is device (or managed) memory - a NULL one is not - or "<who> needs <what> (no CPU path)"
inline int fnn_need_dev(const char *who, std::initializer_list<const void *> ptrs, const char *what = "device pointers") {
    for (const void *p : ptrs)
        if (!p || !fnn_dev_ptr(p)) return fnn_failf(FNN_E_INVALID, "%s needs %s (no CPU path)", who, what);
    return FNN_OK;
}

// regions_class_order -> its device copy (empty for plain labels); what goes wrong is left in the call's status
inline DevBuf upload_order(const int32_t *regions_class_order, int heads, HipCall &c) {
    DevBuf d;
    if (!regions_class_order) return d;
    hipError_t why;
    if (!d.alloc(heads * sizeof(int), &why)) c.r = c.ok() ? why : c.r;
    else c.copy(d.p, regions_class_order, heads * sizeof(int), hipMemcpyHostToDevice);
    return d;
}

// ---- a dtype code -> the element type: f(x) with decltype(x) the type
template <class F> decltype(auto) fnn_by_label(int label_dtype, F &&f) { return label_dtype == FNN_LABEL_U16 ? f(uint16_t()) : f(uint8_t()); }
template <class F> decltype(auto) fnn_by_float(int float_dtype, F &&f) { return float_dtype == FNN_OUT_F32 ? f(float()) : f(f16()); }
