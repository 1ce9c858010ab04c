// resample_torch_common.h - the arithmetic of the torch resampling family, once: what resample_torch.hip (resampled
// images / logits) and export_labels.hip (labels straight from the logits of the network grid) must agree on bit for bit.
#pragma once
#include "fnn_device.h"
#include "../../include/fnn.h"
#include <cmath>

struct RGeo {
    long long in[3], out[3];
    float scale[3];            // (float)in / (float)out
    int sep;                   // the nearest-exact axis or -1
    unsigned plane_blocks;     // blocks of 256 output voxels per x slab
    unsigned plane;            // out[1] * out[2]
};

// the two taps of output index o along axis a and their weights
static __device__ __forceinline__ void axis_taps(const RGeo &g, int a, long long o, long long &i0, long long &i1, float &w0, float &w1) {
    const long long n = g.in[a];
    if (n == g.out[a]) { i0 = i1 = o; w0 = 1.f; w1 = 0.f; return; }
    if (a == g.sep) {
        long long s = (long long)floorf(__fmul_rn((float)o + 0.5f, g.scale[a]));
        s = s > n - 1 ? n - 1 : s;
        i0 = i1 = s; w0 = 1.f; w1 = 0.f;
        return;
    }
    float src = __fmaf_rn(g.scale[a], (float)o + 0.5f, -0.5f);
    src = src < 0.f ? 0.f : src;
    long long f = (long long)src;
    f = f > n - 1 ? n - 1 : f;
    i0 = f; i1 = f + (f < n - 1 ? 1 : 0);
    float l1 = __fsub_rn(src, (float)f);
    l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
    w1 = l1; w0 = __fsub_rn(1.f, l1);
}

struct Taps {
    long long off[8];          // input offsets of the corners, index = 4 * x tap + 2 * y tap + z tap
    float wx0, wx1, wy0, wy1, wz0, wz1;
    long long o;               // output offset inside a channel
    bool live;
};

// the corners and weights of output voxel (ox, oy, oz); o and live are the caller's
static __device__ __forceinline__ void make_taps(const RGeo &g, long long ox, long long oy, long long oz, Taps &t) {
    long long x[2], y[2], z[2];
    axis_taps(g, 0, ox, x[0], x[1], t.wx0, t.wx1);
    axis_taps(g, 1, oy, y[0], y[1], t.wy0, t.wy1);
    axis_taps(g, 2, oz, z[0], z[1], t.wz0, t.wz1);
#pragma unroll
    for (int k = 0; k < 8; ++k) t.off[k] = (x[k >> 2] * g.in[1] + y[(k >> 1) & 1]) * g.in[2] + z[k & 1];
}

// ... of the voxel a thread of a launch of plane_blocks * out[0] blocks of 256 owns
static __device__ __forceinline__ Taps make_taps(const RGeo &g) {
    Taps t;
    const unsigned ox = blockIdx.x / g.plane_blocks;
    const unsigned j = (blockIdx.x - ox * g.plane_blocks) * 256u + threadIdx.x;
    t.live = j < g.plane;
    const unsigned oy = t.live ? j / (unsigned)g.out[2] : 0u;
    const unsigned oz = t.live ? j - oy * (unsigned)g.out[2] : 0u;
    make_taps(g, ox, oy, oz, t);
    t.o = (long long)ox * g.plane + j;
    return t;
}

// w0 * a + w1 * b as torch's CPU kernel rounds it: the second product rounded, then one fused multiply-add - measured
// bit for bit against F.interpolate on float32 inputs (either other order is one step off on about half the values)
static __device__ __forceinline__ float mix(float a, float b, float w0, float w1) { return __fmaf_rn(w0, a, __fmul_rn(w1, b)); }

static __device__ __forceinline__ float blend(const Taps &t, const float (&v)[8]) {
    const float a = mix(mix(v[0], v[1], t.wz0, t.wz1), mix(v[2], v[3], t.wz0, t.wz1), t.wy0, t.wy1);
    const float b = mix(mix(v[4], v[5], t.wz0, t.wz1), mix(v[6], v[7], t.wz0, t.wz1), t.wy0, t.wy1);
    return mix(a, b, t.wx0, t.wx1);
}

// float32 result -> storage type.  For fp16 the conversion must stay an instruction of its own: folded into the last
// fused multiply-add (v_fma_mixlo_f16) the exact sum is rounded to fp16 once, where torch rounds it to float32 first -
// measured as 1e-4 of the values one fp16 step off.  The canonicalize keeps the two apart and costs no instruction.
template <typename T> static __device__ __forceinline__ T store_cast(float v) { return (T)v; }
template <> __device__ __forceinline__ f16 store_cast<f16>(float v) { return (f16)__builtin_canonicalizef(v); }

// the launch geometry of shape -> new_shape, or why it is refused
static inline int rt_geometry(const int64_t shape[4], const int64_t new_shape[3], int sep, RGeo &g, const char **why) {
    g.sep = sep;
    for (int a = 0; a < 3; ++a) {
        g.in[a] = shape[1 + a]; g.out[a] = new_shape[a];
        if (g.in[a] > (1 << 24) || g.out[a] > (1 << 24)) { *why = "an axis longer than 2^24 is not implemented (float32 coordinates)"; return FNN_E_UNSUPPORTED; }
        g.scale[a] = (float)g.in[a] / (float)g.out[a];
    }
    const long long plane = g.out[1] * g.out[2];
    const long long pb = (plane + 255) / 256;
    if (plane >= (1LL << 31) || pb * g.out[0] >= (1LL << 31) || shape[0] >= (1LL << 31)) { *why = "output too large for one launch"; return FNN_E_UNSUPPORTED; }
    g.plane = (unsigned)plane; g.plane_blocks = (unsigned)pb;
    return FNN_OK;
}
