// finalize.hip - from accumulators to results (gfx950): acc / weight sum, inf check, un-pad -> logits, the
// label map straight from the accumulators, the fold ensemble's division, logits -> labels (K10)
#include "output_common.h"
#include <type_traits>

// ----------------------------------------------------------------------------
// normalise + un-pad (+ fold ensembling): channels-last accumulators -> planar logits
// (predict_from_raw_data.py:620-625, :679, :494-500).  One thread = one output voxel.
// ----------------------------------------------------------------------------
template <bool ACC32>
__global__ __launch_bounds__(256) void finalize_kernel(const FinalizeParams p) {
    const long long nbox = p.OX * p.OY * p.OZ;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nbox) return;
    const long long z = i % p.OZ, y = (i / p.OZ) % p.OY, x = i / (p.OZ * p.OY);
    const size_t aelem = acc_voxel_of_output(p, x, y, z) * p.HP;
    const size_t oidx0 = ((size_t)(x + p.out_x) * p.out_Y + (y + p.out_y)) * p.out_Z + (z + p.out_z);
    const size_t oplane = (size_t)p.out_X * p.out_Y * p.out_Z;
    const float wsum = ACC32 ? ((const float *)p.acc)[aelem + p.heads] : (float)((const f16 *)p.acc)[aelem + p.heads];
    bool bad = false;
    for (int ch0 = 0; ch0 < p.heads; ch0 += 4) {
        float a[4];
        if (ACC32) {
            const f32x4 t = *(const f32x4 *)((const float *)p.acc + aelem + ch0);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = t[j];
        } else {
            const f16x4 t = *(const f16x4 *)((const f16 *)p.acc + aelem + ch0);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = (float)t[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int head = ch0 + j;
            if (head >= p.heads) break;
            const float qf = __fdiv_rn(a[j], wsum);
            const size_t oidx = (size_t)head * oplane + oidx0;
            if (p.out_fp32) {
                float *o = (float *)p.out;
                const float rr = ACC32 ? qf : (float)(f16)qf;       // reference-rounding mode rounds to half first
                o[oidx] = p.mode ? o[oidx] + rr : rr;
                bad |= isinf(o[oidx]);
            } else {
                f16 *o = (f16 *)p.out;
                const f16 rr = (f16)qf;
                bad |= isinf((float)rr);
                o[oidx] = p.mode ? (f16)((float)o[oidx] + (float)rr) : rr;
            }
        }
    }
    if (bad) atomicOr(p.inf_flag, 1);
}

// Tiled version for the common aligned case: a workgroup takes 64 consecutive z voxels of one (x, y) row,
// reads their accumulator rows fully coalesced (the rows are contiguous: 64 x HP elements), keeps them in
// LDS, and every thread then produces 16 consecutive z voxels of ONE head - a 32-byte (fp16) contiguous
// piece of the planar output.  The one-thread-per-voxel kernel above read each 128-byte row in sixteen
// 8-byte pieces per lane (64 lines touched per load instruction) and ran at 2.1 TB/s.
template <bool ACC32, bool OUT32>
__global__ __launch_bounds__(256) void finalize_tiled_kernel(const FinalizeParams p) {
    typedef typename std::conditional<ACC32, float, f16>::type AT;
    typedef typename std::conditional<OUT32, float, f16>::type OT;
    constexpr int HP = 64, PITCH = HP + (ACC32 ? 1 : 2);              // elements; odd dword pitch
    __shared__ __attribute__((aligned(16))) AT sT[64 * PITCH + 8];
    const int tid = threadIdx.x;
    const long long tiles_z = (p.OZ + 63) / 64;
    const long long row = blockIdx.x / tiles_z;
    const int z0 = (int)(blockIdx.x % tiles_z) * 64;
    const long long y = row % p.OY, x = row / p.OY;
    const int nz = (int)(p.OZ - z0 < 64 ? p.OZ - z0 : 64);
    const AT *src = (const AT *)p.acc + acc_voxel_of_output(p, x, y, z0) * HP;
    constexpr int EPV = 16 / (int)sizeof(AT);                         // elements per 16-byte piece
    constexpr int PIECES = 64 * HP / EPV;
#pragma unroll
    for (int k = 0; k < PIECES / 256; ++k) {
        const int q = tid + k * 256;
        const int v = q / (HP / EPV), part = q % (HP / EPV);
        const uint4 t = *(const uint4 *)(src + (size_t)(v < nz ? v : 0) * HP + part * EPV);
        AT *d = sT + v * PITCH + part * EPV;                          // rows are not 16-byte aligned: element stores
        const AT *tv = (const AT *)&t;
#pragma unroll
        for (int j = 0; j < EPV; ++j) d[j] = tv[j];
    }
    __syncthreads();
    const int head = tid >> 2, vg = (tid & 3) * 16;
    if (head >= p.heads) return;
    const size_t oplane = (size_t)p.out_X * p.out_Y * p.out_Z;
    OT *o = (OT *)p.out + (size_t)head * oplane + ((size_t)(x + p.out_x) * p.out_Y + (y + p.out_y)) * p.out_Z + (z0 + p.out_z) + vg;
    bool bad = false;
    OT r[16];
    if (p.mode) {
#pragma unroll
        for (int i = 0; i < 16; ++i) r[i] = vg + i < nz ? o[i] : (OT)0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float a = (float)sT[(vg + i) * PITCH + head], wsum = (float)sT[(vg + i) * PITCH + p.heads];
        const float qf = __fdiv_rn(a, wsum);
        if (OUT32) {
            const float rr = ACC32 ? qf : (float)(f16)qf;             // reference-rounding mode rounds to half first
            const float res = p.mode ? (float)r[i] + rr : rr;
            bad |= vg + i < nz && isinf(res);
            r[i] = (OT)res;
        } else {
            const f16 rr = (f16)qf;
            bad |= vg + i < nz && isinf((float)rr);
            r[i] = (OT)(p.mode ? (f16)((float)r[i] + (float)rr) : rr);
        }
    }
    if (vg + 16 <= nz) {
#pragma unroll
        for (int i = 0; i < 16 * (int)sizeof(OT) / 16; ++i) ((uint4 *)o)[i] = ((const uint4 *)r)[i];
    } else {
        for (int i = 0; i < 16; ++i) if (vg + i < nz) o[i] = r[i];
    }
    if (bad) atomicOr(p.inf_flag, 1);
}

int launch_finalize(const FinalizeParams &p, hipStream_t st) {
    const long long n = p.OX * p.OY * p.OZ;
    static const bool no_tiled = fnn_knob("FNN_FINALIZE_V1") != nullptr;           // A-B aid
    // tiled kernel: 64-channel accumulator rows, 16-byte aligned output pieces
    const int osz = p.out_fp32 ? 4 : 2;
    const bool aligned = p.HP == 64 && p.heads < 64 && (p.out_Z * osz) % 16 == 0 && (p.out_z * osz) % 16 == 0 &&
                         ((size_t)p.out % 16) == 0;
    if (!no_tiled && aligned) {
        const long long wgs = p.OX * p.OY * ((p.OZ + 63) / 64);
        const dim3 grid((unsigned)wgs);
        if (p.acc_fp32) {
            if (p.out_fp32) hipLaunchKernelGGL((finalize_tiled_kernel<true, true>), grid, dim3(256), 0, st, p);
            else hipLaunchKernelGGL((finalize_tiled_kernel<true, false>), grid, dim3(256), 0, st, p);
        } else {
            if (p.out_fp32) hipLaunchKernelGGL((finalize_tiled_kernel<false, true>), grid, dim3(256), 0, st, p);
            else hipLaunchKernelGGL((finalize_tiled_kernel<false, false>), grid, dim3(256), 0, st, p);
        }
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    if (p.acc_fp32) hipLaunchKernelGGL(finalize_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(finalize_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}


// Label map straight from the accumulators: the label rule (LabelPick, output_common.h) on acc_h / wsum with the
// reference's rounding (divide, round to fp16) without materialising the logits.
template <bool ACC32, typename LT>
__global__ __launch_bounds__(256) void labels_from_acc_kernel(const FinalizeParams p, LT *labels, const int *order) {
    const long long nbox = p.OX * p.OY * p.OZ;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nbox) return;
    const long long z = i % p.OZ, y = (i / p.OZ) % p.OY, x = i / (p.OZ * p.OY);
    const size_t aelem = acc_voxel_of_output(p, x, y, z) * p.HP;
    const size_t oidx0 = ((size_t)(x + p.out_x) * p.out_Y + (y + p.out_y)) * p.out_Z + (z + p.out_z);
    const float wsum = ACC32 ? ((const float *)p.acc)[aelem + p.heads] : (float)((const f16 *)p.acc)[aelem + p.heads];
    LabelPick pick;
    bool bad = false;
    for (int h = 0; h < p.heads; ++h) {
        const float a = ACC32 ? ((const float *)p.acc)[aelem + h] : (float)((const f16 *)p.acc)[aelem + h];
        const float v = (float)(f16)__fdiv_rn(a, wsum);
        bad |= isinf(v);
        pick.feed(h, v);
    }
    labels[oidx0] = (LT)pick.label(order);
    if (bad) atomicOr(p.inf_flag, 1);
}

// The same with G = 2^LOG_G consecutive lanes per voxel, each lane on 8 channels (one 16-byte piece of an fp16
// accumulator line, two of an fp32 one): a wave instruction then reads 64 / G whole voxel lines - contiguous along z -
// instead of 2 bytes out of 64 different lines, 61 times over (the one-thread-per-voxel form above re-fetched every
// line many times: 75 ms for the 17 GB of a 512^3 x 61 volume, this one runs at the HBM rate).  The lanes' partial
// picks are merged (LabelPick::merge), so "first maximum / first NaN wins" and "last region above the threshold wins"
// are exactly the sequential rule.
template <bool ACC32, typename LT, int LOG_G>
__global__ __launch_bounds__(256) void labels_from_acc_coop_kernel(const FinalizeParams p, LT *labels, const int *order) {
    constexpr int G = 1 << LOG_G;
    const long long nbox = p.OX * p.OY * p.OZ;
    const long long gt = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long iv = gt >> LOG_G;
    const int piece = (int)(gt & (G - 1));
    const long long i = iv < nbox ? iv : nbox - 1;                   // surplus lanes redo the last voxel (no store)
    const long long z = i % p.OZ, y = (i / p.OZ) % p.OY, x = i / (p.OZ * p.OY);
    const size_t aelem = acc_voxel_of_output(p, x, y, z) * p.HP;
    const int c0 = piece * 8;
    float v[8];
    const bool have = c0 < p.HP;
    if (ACC32) {
        const float4 a = have ? *(const float4 *)((const float *)p.acc + aelem + c0) : make_float4(0, 0, 0, 0);
        const float4 b = have ? *(const float4 *)((const float *)p.acc + aelem + c0 + 4) : make_float4(0, 0, 0, 0);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        f16x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
        if (have) a = *(const f16x8 *)((const f16 *)p.acc + aelem + c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)a[j];
    }
    // the weight sum sits in channel `heads`: broadcast from the lane that holds it
    const int wl = p.heads >> 3, wj = p.heads & 7;
    float wsum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j == wj) wsum = v[j];
    wsum = __shfl(wsum, (threadIdx.x & 63 & ~(G - 1)) + wl, 64);
    // this lane's pick over its channels, then the voxel's lanes merge theirs
    LabelPick pick;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int h = c0 + j;
        if (h < p.heads) {
            const float q = (float)(f16)__fdiv_rn(v[j], wsum);
            bad |= isinf(q);
            pick.feed(h, q);
        }
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) pick.merge(pick.across(m));
    if (piece == 0 && iv < nbox) {
        const size_t oidx0 = ((size_t)(x + p.out_x) * p.out_Y + (y + p.out_y)) * p.out_Z + (z + p.out_z);
        labels[oidx0] = (LT)pick.label(order);
    }
    if (bad && iv < nbox) atomicOr(p.inf_flag, 1);
}

template <bool ACC32, typename LT>
static void launch_labels_coop(const FinalizeParams &p, void *labels, const int *order, int log_g, hipStream_t st) {
    const long long n = (p.OX * p.OY * p.OZ) << log_g;
    const dim3 grid((unsigned)((n + 255) / 256));
    switch (log_g) {
        case 0: hipLaunchKernelGGL((labels_from_acc_coop_kernel<ACC32, LT, 0>), grid, dim3(256), 0, st, p, (LT *)labels, order); break;
        case 1: hipLaunchKernelGGL((labels_from_acc_coop_kernel<ACC32, LT, 1>), grid, dim3(256), 0, st, p, (LT *)labels, order); break;
        case 2: hipLaunchKernelGGL((labels_from_acc_coop_kernel<ACC32, LT, 2>), grid, dim3(256), 0, st, p, (LT *)labels, order); break;
        case 3: hipLaunchKernelGGL((labels_from_acc_coop_kernel<ACC32, LT, 3>), grid, dim3(256), 0, st, p, (LT *)labels, order); break;
        case 4: hipLaunchKernelGGL((labels_from_acc_coop_kernel<ACC32, LT, 4>), grid, dim3(256), 0, st, p, (LT *)labels, order); break;
        default: hipLaunchKernelGGL((labels_from_acc_coop_kernel<ACC32, LT, 5>), grid, dim3(256), 0, st, p, (LT *)labels, order); break;
    }
}

int launch_labels_from_acc(const FinalizeParams &p, void *labels, int label_u16, const int *order, hipStream_t st) {
    // uint8 labels (<= 256 classes: <= 32 lanes per voxel): the cooperative kernel; uint16 labels (what more classes need): one
    // lane per voxel.  (Round 3: the other twelve + two combinations were kernels only a knob or a raw ABI call reached.)
    int log_g = 0;
    while ((8 << log_g) < p.HP) ++log_g;                                         // lanes per voxel: HP / 8 rounded up to 2^k
    const long long nvox = p.OX * p.OY * p.OZ;
    if (!label_u16) {
        if (log_g > 5 || (nvox << log_g) >= (1LL << 39)) return -1;
        if (p.acc_fp32) launch_labels_coop<true, uint8_t>(p, labels, order, log_g, st);
        else launch_labels_coop<false, uint8_t>(p, labels, order, log_g, st);
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    const dim3 grid((unsigned)((nvox + 255) / 256));
    if (p.acc_fp32) hipLaunchKernelGGL((labels_from_acc_kernel<true, uint16_t>), grid, dim3(256), 0, st, p, (uint16_t *)labels, order);
    else hipLaunchKernelGGL((labels_from_acc_kernel<false, uint16_t>), grid, dim3(256), 0, st, p, (uint16_t *)labels, order);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

__global__ __launch_bounds__(256) void scale_output_kernel(void *out, int out_fp32, long long n, int divisor) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (out_fp32) ((float *)out)[i] /= (float)divisor;
    else ((f16 *)out)[i] = (f16)((float)((f16 *)out)[i] / (float)divisor);
}

int launch_scale_output(void *out, int out_fp32, long long n, int divisor, int *, hipStream_t st) {
    hipLaunchKernelGGL(scale_output_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out, out_fp32, n, divisor);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ----------------------------------------------------------------------------
// logits [heads][n_vox] -> label map (argmax or regions: LabelPick, output_common.h)
// ----------------------------------------------------------------------------
template <typename LT>
__global__ __launch_bounds__(256) void argmax_kernel(const void *logits, int fp32, int heads, long long nvox, LT *labels,
                                                     const int *order) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvox) return;
    LabelPick pick;
    for (int h = 0; h < heads; ++h) {
        const float v = fp32 ? ((const float *)logits)[(size_t)h * nvox + i] : (float)((const f16 *)logits)[(size_t)h * nvox + i];
        pick.feed(h, v);
    }
    labels[i] = (LT)pick.label(order);
}

int launch_argmax(const void *logits, int fp32, int heads, long long nvox, void *labels, int label_u16, const int *order,
                  hipStream_t st) {
    const dim3 grid((unsigned)((nvox + 255) / 256));
    if (label_u16) hipLaunchKernelGGL(argmax_kernel<uint16_t>, grid, dim3(256), 0, st, logits, fp32, heads, nvox, (uint16_t *)labels, order);
    else hipLaunchKernelGGL(argmax_kernel<uint8_t>, grid, dim3(256), 0, st, logits, fp32, heads, nvox, (uint8_t *)labels, order);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
