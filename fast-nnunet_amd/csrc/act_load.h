// act_load.h - how the kernels between and behind the convs read an activation tensor: the producer's InstanceNorm rows
// as (scale, shift) pairs in LDS, a raw fragment normalised and activated on load (tconv.hip, head.hip, body.hip).
#pragma once
#include "fnn_device.h"

// division by a workgroup-uniform divisor through its float reciprocal, exact for 0 <= v < 2^24
// (conv_common.h's small_div is the form for v < 2^16 with plain multiplies: other instructions, another range - both stay)
static __device__ __forceinline__ int recip_div(int v, int d, float rcp) {
    int q = (int)((float)v * rcp);
    q -= ((int)__umul24(q, d) > v);                            // 24-bit multiplies: full rate (v_mul_lo_u32 is quarter rate)
    q += ((int)__umul24(q + 1, d) <= v);
    return q;
}

static __device__ __forceinline__ void load_scale_shift(const SrcDesc &s, int n, float2 *sSS, int tid, int nthreads) {
    for (int c = tid; c < s.C; c += nthreads)
        sSS[c] = s.ss ? make_float2(s.ss[(size_t)(2 * n) * s.C + c], s.ss[(size_t)(2 * n + 1) * s.C + c]) : make_float2(1.f, 0.f);
}

// Normalise + LeakyReLU of a raw fragment of 8 channels starting at c0 (zero beyond the source's channels).
static __device__ __forceinline__ f16x8 norm_act_frag(const SrcDesc &s, const f16x8 &x, int c0, const float2 *sSS) {
    const bool live = c0 < s.C;
    const int cc = live ? c0 : 0;
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float2 ss = sSS[cc + j]; sc[j] = ss.x; sh[j] = ss.y; }
    f16x8 o = fnn_norm8(x, sc, sh);
    o = __builtin_elementwise_max(o, o * (f16)s.slope);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = live ? o[j] : (f16)0.f;
    return o;
}

// Activation fragment (MFMA B operand) of 16 voxels x 32 channels, read from a
// channels-last tensor with the producer's norm + LeakyReLU applied.
// `item`: element offset of the batch item when `vox` counts inside it - the form that honours the source's layout
// (fnn_device.h, SrcDesc: v * vs + (c >> 4) * cs + (c & 15)); with item = 0 and a global voxel index the source must be
// channels-last (the seg-head kernels' feature tensors are).
static __device__ __forceinline__ f16x8 load_act_frag(const SrcDesc &s, size_t vox, bool vox_ok, int c0,
                                                      const float2 *sSS, size_t item = 0) {
    // unconditional load from a clamped (always valid) address, zeroed afterwards: a per-lane branch around
    // the load makes hipcc wait for it immediately and serialises the loads of a k-step
    const bool live = vox_ok && c0 < s.C;
    const int cc = c0 < s.C ? c0 : 0;
    const f16x8 x = *(const f16x8 *)(s.ptr + item + (vox_ok ? vox : 0) * FNN_VS(s) + (cc >> 4) * FNN_CS(s) + (cc & 15));
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float2 ss = sSS[cc + j]; sc[j] = ss.x; sh[j] = ss.y; }
    f16x8 o = fnn_norm8(x, sc, sh);
    o = __builtin_elementwise_max(o, o * (f16)s.slope);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = live ? o[j] : (f16)0.f;
    return o;
}

