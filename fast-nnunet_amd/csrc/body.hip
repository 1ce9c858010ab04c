// body.hip - the small kernels of a patch's way through the network, between the convs (gfx950):
//   patch_input_kernel     patch windows of the volume -> the stem's fp16 input
//   stats_finalize_kernel  InstanceNorm statistics -> (scale, shift) rows;  fss_to_ssh_kernel: a caller's rows -> fp16
//   avgpool_kernel, combine_kernel, combine_pool_kernel   the residual encoder's skip pooling and closing add
//   region_copy_kernel     sub-blocks of kept activations <-> one message (fnn_pack_regions / fnn_unpack_regions)
//   pad_volume_kernel      zero-pad a volume smaller than the patch
#include "act_load.h"

// InstanceNorm statistics -> per (n, channel) (scale, shift):  y = x * scale + shift
//   mean = sum / count, var = sumsq / count - mean^2 (biased, like torch), scale = gamma / sqrt(var + eps)
// The producer filled `nrep` rows per item: 8 replicas (atomics) or one row per tile (plain stores, up to a few
// hundred).  A workgroup takes 16 channels of one item: thread = (row lane 0..63, channel), rows strided by 64, the 64
// partial sums of a channel meet in LDS.  Sums of fp16-valued numbers in double are exact: any order gives the same bits.
__global__ __launch_bounds__(1024) void stats_finalize_kernel(const StatsFinalizeParams p) {
    constexpr int RL = 64;                                            // row lanes: 1024 threads = 64 x 16 channels
    __shared__ double sred[RL][16][2];
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.y * 16 + cl, n = blockIdx.x;
    double s1 = 0, s2 = 0;
    if (c < p.C) {
        const double *st = p.stats + ((size_t)n * p.nrep * p.C + c) * 2;
#pragma unroll 4
        for (int r = rl; r < p.nrep; r += RL) {                       // independent loads: several in flight
            const double2 v = *(const double2 *)(st + (size_t)r * p.C * 2);
            s1 += v.x; s2 += v.y;
        }
    }
    sred[rl][cl][0] = s1; sred[rl][cl][1] = s2;
    __syncthreads();
    if (rl >= 4) return;                                              // 4 lanes x 16 rows each, then 4 -> 1
    s1 = 0; s2 = 0;
#pragma unroll
    for (int r = 0; r < RL / 4; ++r) { s1 += sred[rl * (RL / 4) + r][cl][0]; s2 += sred[rl * (RL / 4) + r][cl][1]; }
    __syncthreads();
    sred[rl][cl][0] = s1; sred[rl][cl][1] = s2;
    __syncthreads();
    if (rl != 0 || c >= p.C) return;
    s1 = sred[0][cl][0] + sred[1][cl][0] + sred[2][cl][0] + sred[3][cl][0];
    s2 = sred[0][cl][1] + sred[1][cl][1] + sred[2][cl][1] + sred[3][cl][1];
    const double mean = s1 * (double)p.inv_count;
    double var = s2 * (double)p.inv_count - mean * mean;
    var = var > 0 ? var : 0;
    const float rstd = (float)(1.0 / sqrt(var + (double)p.eps));
    const float sc = p.gamma[c] * rstd;
    const float sh = p.beta[c] - (float)mean * sc;
    p.ss[(size_t)(2 * n) * p.C + c] = sc;
    p.ss[(size_t)(2 * n + 1) * p.C + c] = sh;
    if (p.ssh) {                                                      // fp16 rows for the staging threads (SrcDesc::ssh)
        f16 *h = (f16 *)p.ssh + ((size_t)n * p.C + (c & ~7)) * 2 + (c & 7);
        h[0] = (f16)sc;
        h[8] = (f16)sh;
    }
}

int launch_stats_finalize(const StatsFinalizeParams &p, int N, hipStream_t st) {
    hipLaunchKernelGGL(stats_finalize_kernel, dim3(N, (p.C + 15) / 16), dim3(1024), 0, st, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// (scale, shift) rows of kept patch activations, fp32 [items][2][C] as the C ABI hands them over (fnn_patch_features) ->
// the fp16 staging layout stats_finalize_kernel writes next to its fp32 rows (SrcDesc::ssh): the same roundings
__global__ __launch_bounds__(256) void fss_to_ssh_kernel(const float *fss, unsigned short *ssh, long long n, int C) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;      // (item, channel)
    if (i >= n) return;
    const long long item = i / C;
    const int c = (int)(i - item * C);
    f16 *h = (f16 *)ssh + (item * C + (c & ~7)) * 2 + (c & 7);
    h[0] = (f16)fss[item * 2 * C + c];
    h[8] = (f16)fss[item * 2 * C + C + c];
}

// fnn_pack_regions / fnn_unpack_regions (include/fnn.h): the sub-blocks of kept patch activations that one neighbour
// needs <-> one contiguous message, a launch per peer and direction instead of a strided torch copy per sub-block.
// blockIdx.y = region, the region's 16-byte vectors grid-strided over blockIdx.x; a voxel record is C / 8 vectors.
template <bool PACK>
__global__ __launch_bounds__(256) void region_copy_kernel(char *feat, const int *regions, char *message, long long n_slots,
                                                          int PH, int PW, long long slot_bytes, int vpv) {
    const int *rc = regions + (size_t)blockIdx.y * 10;
    const int ev = rc[0], slot = rc[1], l0 = rc[2], l1 = rc[3], l2 = rc[4];
    const int d0 = rc[5] - l0, d1 = rc[6] - l1, d2 = rc[7] - l2;
    const long long nvec = (long long)d0 * d1 * d2 * vpv;
    char *sp = feat + ((long long)ev * n_slots + slot) * slot_bytes;
    char *mp = message + (long long)rc[8] * 16;
    const int row = d2 * vpv;                                            // vectors per w row of the block: contiguous in both
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long long)gridDim.x * 256) {
        const long long rw = i / row;
        const int c = (int)(i - rw * row);
        const int h = (int)(rw % d1), dd = (int)(rw / d1);
        char *fp = sp + ((((long long)(l0 + dd) * PH + (l1 + h)) * PW + l2) * vpv + c) * 16;
        if (PACK) *(fnn_u32x4r *)(mp + i * 16) = *(const fnn_u32x4r *)fp;
        else *(fnn_u32x4r *)fp = *(const fnn_u32x4r *)(mp + i * 16);
    }
}

int launch_region_copy(void *feat, long long n_slots, const int *regions, int n, void *message, int PD, int PH, int PW, int C,
                       bool pack, hipStream_t st) {
    if (n <= 0) return 0;
    const int vpv = C / 8;                                               // 16-byte vectors per voxel record
    const long long slot_bytes = (long long)PD * PH * PW * C * 2;
    const dim3 grid(128, (unsigned)n);                                   // (a face region of a 160 x 96 x 96 patch: ~10^5 vectors)
    if (pack) hipLaunchKernelGGL(region_copy_kernel<true>, grid, dim3(256), 0, st, (char *)feat, regions, (char *)message, n_slots, PH, PW, slot_bytes, vpv);
    else hipLaunchKernelGGL(region_copy_kernel<false>, grid, dim3(256), 0, st, (char *)feat, regions, (char *)message, n_slots, PH, PW, slot_bytes, vpv);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_fss_to_ssh(const float *fss, unsigned short *ssh, long long items, int C, hipStream_t st) {
    const long long n = items * C;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(fss_to_ssh_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, fss, ssh, n, C);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ----------------------------------------------------------------------------
// residual-encoder helpers (BasicBlockD of dynamic_network_architectures' ResidualEncoderUNet, instantiated
// by the reference at nnUNetDistillationTrainer.py:248-266): one thread = one voxel x 8 channels
// ----------------------------------------------------------------------------
static __device__ __forceinline__ void apply8(const SrcDesc &s, int n, int c0, const f16x8 &x, float (&y)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float v = (float)x[j];
        if (s.ss) v = fmaf(v, s.ss[(size_t)(2 * n) * s.C + c0 + j], s.ss[(size_t)(2 * n + 1) * s.C + c0 + j]);
        y[j] = leaky(v, s.slope);
    }
}

// Patch windows of the fp32 volume -> fp16 [N][PD][PH][PW][Cpad] (x rounded to fp16 once: the engine's contract for every
// conv operand).  Thread = (voxel, 8-channel group); a wave's 64 voxels are consecutive along z, so each of its (up to 8)
// channel-plane reads is 256 contiguous bytes and its 16-byte stores tile whole records.  The patch coordinates come from
// 32-bit arithmetic (a patch has < 2^31 voxels); mirroring is the coordinate P - 1 - v.  (Measured, round 6: four voxels per thread with all
// their loads in flight - 2 channels at 20 x 320 x 256 915 -> 690 us, 14 channels at 128^3 1765 -> 1670 us, but 4 channels at 128^3 1258 -> 1337 us and one
// channel at 512^2 152 -> 275 us: profiles/r06_plan_sweep_patch_input_u4.txt - not kept.)  Replaces the patch slicing
// `data[sl]` of predict_from_raw_data.py:560-566 for stems that run on the MFMA conv kernels (engine.hip, Layer::GATHER).
__global__ __launch_bounds__(256) void patch_input_kernel(const PatchInputParams p) {
    const unsigned pvox = (unsigned)p.PD * p.PH * p.PW;
    const unsigned cg = (unsigned)(p.Cpad >> 3);
    const unsigned n = blockIdx.y / cg, g = blockIdx.y % cg;
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= pvox) return;
    const unsigned w = v % (unsigned)p.PW, t = v / (unsigned)p.PW, h = t % (unsigned)p.PH, d = t / (unsigned)p.PH;
    const long long x = p.origins[n * 3 + 0] + (p.flip_d ? p.PD - 1 - (int)d : (int)d);
    const long long y = p.origins[n * 3 + 1] + (p.flip_h ? p.PH - 1 - (int)h : (int)h);
    const long long z = p.origins[n * 3 + 2] + (p.flip_w ? p.PW - 1 - (int)w : (int)w);
    const float *src = p.vol + (size_t)n * p.vol_batch_stride + (size_t)((x * p.Y + y) * p.Z + z);
    const size_t plane = (size_t)p.X * p.Y * p.Z;
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = (int)g * 8 + j;
        o[j] = c < p.C ? (f16)src[(size_t)c * plane] : (f16)0.f;
    }
    const int c0 = (int)g * 8;
    const size_t vs = p.out_vs ? (size_t)p.out_vs : (size_t)p.Cpad;
    const size_t cs = p.out_vs ? (size_t)p.out_cs : 16;
    *(f16x8 *)(p.out + (size_t)n * pvox * p.Cpad + (size_t)v * vs + (size_t)(c0 >> 4) * cs + (c0 & 15)) = o;
}

int launch_patch_input(const PatchInputParams &p, hipStream_t st) {
    const unsigned pvox = (unsigned)p.PD * p.PH * p.PW;
    fnn_note_kernel("patch_input_kernel");
    hipLaunchKernelGGL(patch_input_kernel, dim3((pvox + 255) / 256, (unsigned)(p.N * (p.Cpad >> 3))), dim3(256), 0, st, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// skip path of a strided block: AvgPool3d(stride, stride) of the (transformed) block input.  Thread -> (voxel, 8-channel
// group): the group runs fastest for a channels-last output, the voxel (inside a 16-channel chunk) for a chunk-major
// one, so that a wave's stores are contiguous either way; element addresses by the one formula of fnn_device.h.
__global__ __launch_bounds__(256) void avgpool_kernel(const PoolParams p) {
    const int Do = p.Di / p.sd, Ho = p.Hi / p.sh, Wo = p.Wi / p.sw;
    const int cg = p.src.C >> 3;
    const long long ovox = (long long)Do * Ho * Wo;
    const long long total = (long long)p.N * ovox * cg;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int g, n;
    long long v;                                                          // output voxel inside item n
    if (p.out_vs) {                                                       // chunk-major: (n, chunk, voxel, half)
        const int half = (int)(i & 1);
        long long t = i >> 1;
        v = t % ovox; t /= ovox;
        const int chunk = (int)(t % (cg >> 1));
        n = (int)(t / (cg >> 1));
        g = chunk * 2 + half;
    } else {
        g = (int)(i % cg);
        const long long t = i / cg;
        v = t % ovox;
        n = (int)(t / ovox);
    }
    const int ow = (int)(v % Wo), oh = (int)((v / Wo) % Ho), od = (int)(v / ((long long)Wo * Ho));
    const int c0 = g * 8;
    const f16 *srcn = p.src.ptr + (size_t)n * p.Di * p.Hi * p.Wi * p.src.C + (c0 >> 4) * FNN_CS(p.src) + (c0 & 15);
    const int vs = FNN_VS(p.src);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int a = 0; a < p.sd; ++a)
        for (int b = 0; b < p.sh; ++b)
            for (int c = 0; c < p.sw; ++c) {
                const size_t vin = (((size_t)od * p.sd + a) * p.Hi + oh * p.sh + b) * p.Wi + ow * p.sw + c;
                const f16x8 x = *(const f16x8 *)(srcn + vin * vs);
                float y[8];
                apply8(p.src, n, c0, x, y);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += y[j];
            }
    const float inv = 1.f / (float)(p.sd * p.sh * p.sw);
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)(acc[j] * inv);
    *(f16x8 *)(p.out + (size_t)n * ovox * p.src.C + (size_t)v * (p.out_vs ? p.out_vs : p.src.C) + (c0 >> 4) * (p.out_vs ? p.out_cs : 16LL) + (c0 & 15)) = o;
}

int launch_avgpool(const PoolParams &p, hipStream_t st) {
    const long long total = (long long)p.N * (p.Di / p.sd) * (p.Hi / p.sh) * (p.Wi / p.sw) * (p.src.C >> 3);
    fnn_note_kernel("avgpool_kernel");
    hipLaunchKernelGGL(avgpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// y = LeakyReLU(T_a(a) + T_b(b)): the closing add of a residual block, stored as final values.  Either layout on every
// operand (the one address formula of fnn_device.h).  grid.y = batch item (x 16-channel chunk for a chunk-major output),
// grid.x walks the item's 16-byte vectors in the output's storage order, FNN_CMB_U of them per thread at a stride of
// 256: all index arithmetic is 32-bit (round 2's one-vector-per-thread form spent its time in two 64-bit divisions per
// thread and ran at 2.5 TB/s) and the 2 x FNN_CMB_U loads of a thread are in flight together.
#define FNN_CMB_U 4
__global__ __launch_bounds__(256) void combine_kernel(const CombineParams p) {
    const unsigned cg = (unsigned)(p.a.C >> 3);
    const unsigned per = p.out_vs ? 2u : cg;                              // vectors per voxel inside one grid row
    const unsigned rowlen = (unsigned)p.vox * per;
    const unsigned n = p.out_vs ? blockIdx.y / (cg >> 1) : blockIdx.y;
    const unsigned chunk = p.out_vs ? blockIdx.y % (cg >> 1) : 0u;
    const bool fixed = p.out_vs || (256u % cg) == 0u;                     // the thread's channel group is the same for every u
    const size_t item = (size_t)n * p.vox * p.a.C;
    const unsigned j0 = blockIdx.x * (256u * FNN_CMB_U) + threadIdx.x;
    f16x8 xa[FNN_CMB_U], xb[FNN_CMB_U];
    unsigned vv[FNN_CMB_U], cc[FNN_CMB_U];
#pragma unroll
    for (int u = 0; u < FNN_CMB_U; ++u) {
        const unsigned j = j0 + 256u * u;
        const unsigned jj = j < rowlen ? j : rowlen - 1;                  // clamped, always valid address
        const unsigned g = p.out_vs ? chunk * 2 + (jj & 1u) : jj % cg;
        vv[u] = p.out_vs ? jj >> 1 : jj / cg;
        cc[u] = g * 8;
        xa[u] = *(const f16x8 *)(p.a.ptr + item + (size_t)vv[u] * FNN_VS(p.a) + (cc[u] >> 4) * FNN_CS(p.a) + (cc[u] & 15));
        xb[u] = *(const f16x8 *)(p.b.ptr + item + (size_t)vv[u] * FNN_VS(p.b) + (cc[u] >> 4) * FNN_CS(p.b) + (cc[u] & 15));
    }
    float sa[8], ha[8], sb[8], hb[8];
#pragma unroll
    for (int u = 0; u < FNN_CMB_U; ++u) {
        if (u == 0 || !fixed) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                sa[j] = p.a.ss ? p.a.ss[(size_t)(2 * n) * p.a.C + cc[u] + j] : 1.f;
                ha[j] = p.a.ss ? p.a.ss[(size_t)(2 * n + 1) * p.a.C + cc[u] + j] : 0.f;
                sb[j] = p.b.ss ? p.b.ss[(size_t)(2 * n) * p.b.C + cc[u] + j] : 1.f;
                hb[j] = p.b.ss ? p.b.ss[(size_t)(2 * n + 1) * p.b.C + cc[u] + j] : 0.f;
            }
        }
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float ya = (float)xa[u][j], yb = (float)xb[u][j];
            if (p.a.ss) ya = fmaf(ya, sa[j], ha[j]);
            if (p.b.ss) yb = fmaf(yb, sb[j], hb[j]);
            o[j] = (f16)leaky(leaky(ya, p.a.slope) + leaky(yb, p.b.slope), p.slope);
        }
        if (j0 + 256u * u < rowlen)
            *(f16x8 *)(p.out + item + (size_t)vv[u] * (p.out_vs ? p.out_vs : p.a.C) + (cc[u] >> 4) * (p.out_vs ? p.out_cs : 16LL) +
                       (cc[u] & 15)) = o;
    }
}

// The closing add of a stage's last block AND the next stage's skip-path pooling in one pass (round 5): thread = (pooled
// voxel, 8-channel group) like avgpool_kernel; it forms the sd x sh x sw block outputs under its pooled voxel with
// combine_kernel's arithmetic, stores them, and averages the fp16-ROUNDED values in avgpool_kernel's order (fp32 sum over
// d, h, w ascending, times 1 / count, one rounding): both tensors carry the bits the two kernels wrote.
template <int SD, int SH, int SW>
__global__ __launch_bounds__(256) void combine_pool_kernel(const CombineParams p) {
    const int Do = p.D / SD, Ho = p.H / SH, Wo = p.W / SW;
    const int cg = p.a.C >> 3;
    const long long ovox = (long long)Do * Ho * Wo;
    const long long total = (long long)p.N * ovox * cg;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int g, n;
    long long v;                                                          // pooled voxel inside item n
    if (p.pool_vs) {                                                      // chunk-major pooled tensor: (n, chunk, voxel, half)
        const int half = (int)(i & 1);
        long long t = i >> 1;
        v = t % ovox; t /= ovox;
        const int chunk = (int)(t % (cg >> 1));
        n = (int)(t / (cg >> 1));
        g = chunk * 2 + half;
    } else {
        g = (int)(i % cg);
        const long long t = i / cg;
        v = t % ovox;
        n = (int)(t / ovox);
    }
    const int ow = (int)(v % Wo), oh = (int)((v / Wo) % Ho), od = (int)(v / ((long long)Wo * Ho));
    const int c0 = g * 8;
    const size_t item = (size_t)n * p.vox * p.a.C;
    const f16 *pa = p.a.ptr + item + (size_t)(c0 >> 4) * FNN_CS(p.a) + (c0 & 15);
    const f16 *pb = p.b.ptr + item + (size_t)(c0 >> 4) * FNN_CS(p.b) + (c0 & 15);
    f16 *po = p.out + item + (size_t)(c0 >> 4) * (p.out_vs ? p.out_cs : 16LL) + (c0 & 15);
    const unsigned vsa = (unsigned)FNN_VS(p.a), vsb = (unsigned)FNN_VS(p.b), vso = (unsigned)(p.out_vs ? p.out_vs : p.a.C);
    constexpr int NV = SD * SH * SW;
    // every load of the thread leaves before the first use: 2 NV 16-byte loads in flight (the runtime-bounded loops of the
    // first form waited for four at a time and ran at half the rate of the two kernels it replaces)
    f16x8 xa[NV], xb[NV];
    unsigned vin[NV];                                                     // voxel index inside the item (< 2^31 / C: launch_combine)
#pragma unroll
    for (int a = 0; a < SD; ++a)
#pragma unroll
        for (int b = 0; b < SH; ++b)
#pragma unroll
            for (int c = 0; c < SW; ++c) {
                const int k = (a * SH + b) * SW + c;
                vin[k] = (unsigned)(((od * SD + a) * p.H + oh * SH + b) * p.W + ow * SW + c);
                xa[k] = *(const f16x8 *)(pa + (size_t)vin[k] * vsa);
                xb[k] = *(const f16x8 *)(pb + (size_t)vin[k] * vsb);
            }
    float sa[8], ha[8], sb[8], hb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sa[j] = p.a.ss ? p.a.ss[(size_t)(2 * n) * p.a.C + c0 + j] : 1.f;
        ha[j] = p.a.ss ? p.a.ss[(size_t)(2 * n + 1) * p.a.C + c0 + j] : 0.f;
        sb[j] = p.b.ss ? p.b.ss[(size_t)(2 * n) * p.b.C + c0 + j] : 1.f;
        hb[j] = p.b.ss ? p.b.ss[(size_t)(2 * n + 1) * p.b.C + c0 + j] : 0.f;
    }
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {                                        // (d, h, w ascending: avgpool_kernel's order of summation)
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float ya = (float)xa[k][j], yb = (float)xb[k][j];
            if (p.a.ss) ya = fmaf(ya, sa[j], ha[j]);
            if (p.b.ss) yb = fmaf(yb, sb[j], hb[j]);
            o[j] = (f16)leaky(leaky(ya, p.a.slope) + leaky(yb, p.b.slope), p.slope);
            acc[j] += (float)o[j];
        }
        *(f16x8 *)(po + (size_t)vin[k] * vso) = o;
    }
    const float inv = 1.f / (float)NV;
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)(acc[j] * inv);
    *(f16x8 *)(p.pool_out + (size_t)n * ovox * p.a.C + (size_t)v * (p.pool_vs ? p.pool_vs : p.a.C) + (c0 >> 4) * (p.pool_vs ? p.pool_cs : 16LL) + (c0 & 15)) = o;
}

// the fused form serves the strides the networks use: (2, 2, 2) and (1, 2, 2), sizes that are multiples of them
bool combine_pool_ok(int D, int H, int W, int sd, int sh, int sw) {
    return sh == 2 && sw == 2 && (sd == 1 || sd == 2) && D % sd == 0 && H % 2 == 0 && W % 2 == 0 && (long long)D * H * W < (1LL << 26);
}

int launch_combine(const CombineParams &p, hipStream_t st) {
    const int cg = p.a.C >> 3;
    if (p.pool_out) {
        if (!combine_pool_ok(p.D, p.H, p.W, p.psd, p.psh, p.psw) || (long long)p.D * p.H * p.W != p.vox) return -1;
        const long long total = (long long)p.N * (p.D / p.psd) * (p.H / p.psh) * (p.W / p.psw) * cg;
        const dim3 grid((unsigned)((total + 255) / 256));
        fnn_note_kernel("combine_pool_kernel");
        if (p.psd == 2) hipLaunchKernelGGL((combine_pool_kernel<2, 2, 2>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((combine_pool_kernel<1, 2, 2>), grid, dim3(256), 0, st, p);
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    const long long rowlen = p.vox * (p.out_vs ? 2 : cg);
    const long long rows = (long long)p.N * (p.out_vs ? cg >> 1 : 1);
    if (rowlen >= (1LL << 32) - 256 * FNN_CMB_U || rows > 65535) return -1;
    fnn_note_kernel("combine_kernel");
    hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((rowlen + 256 * FNN_CMB_U - 1) / (256 * FNN_CMB_U)), (unsigned)rows), dim3(256), 0,
                       st, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ----------------------------------------------------------------------------
// zero-pad a volume that is smaller than the patch (pad_nd_image use at :657)
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pad_volume_kernel(const float *src, float *dst, int C, long long sx, long long sy,
                                                         long long sz, long long dx, long long dy, long long dz,
                                                         long long lx, long long ly, long long lz) {
    const long long n = (long long)C * dx * dy * dz;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long z = i % dz, y = (i / dz) % dy, x = (i / (dz * dy)) % dx, c = i / (dz * dy * dx);
    const long long ux = x - lx, uy = y - ly, uz = z - lz;
    float v = 0.f;
    if (ux >= 0 && ux < sx && uy >= 0 && uy < sy && uz >= 0 && uz < sz) v = src[((c * sx + ux) * sy + uy) * sz + uz];
    dst[i] = v;
}

int launch_pad_volume(const float *src, float *dst, int C, const long long s[3], const long long d[3],
                      const long long lo[3], hipStream_t st) {
    const long long n = (long long)C * d[0] * d[1] * d[2];
    hipLaunchKernelGGL(pad_volume_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, dst, C, s[0], s[1], s[2],
                       d[0], d[1], d[2], lo[0], lo[1], lo[2]);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
