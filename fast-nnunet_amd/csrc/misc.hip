// misc.hip - the remaining gfx950 kernels of the sliding-window path:
//   tconv_mfma_kernel   ConvTranspose3d(kernel = stride)  
//   seg_head_kernel     1x1x1 seg head + Gaussian weighting + accumulate into
//                       the HBM-resident volume accumulators (K6 + K7)
//   patch_acc_kernel    mirrored-evaluation mean -> accumulators (K9 path)
//   finalize_kernel     acc / weight-sum, inf check, un-pad (K8)
//   argmax_kernel       logits -> labels (K10)
#include "fnn_device.h"
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>
#include <cstdlib>
#include <cstring>

const char *fnn_knob(const char *name) {
    static const bool on = [] { const char *v = getenv("FNN_KNOBS"); return v && strcmp(v, "0") != 0; }();
    return on ? getenv(name) : nullptr;
}

static thread_local std::vector<std::string> *g_klog = nullptr;
void fnn_klog_target(void *v) { g_klog = (std::vector<std::string> *)v; }
void fnn_note_kernel(const char *fmt, ...) {
    if (!g_klog) return;
    char buf[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_klog->push_back(buf);
}
#include <cstdlib>
#include <type_traits>

// a + round(t * g): the product is rounded before the sum like the reference's `pred *= g; acc += pred`.  With the
// multiply next to the add hipcc contracts the pair into an fma (even through __fmul_rn / __fadd_rn): contraction is
// switched off for this block.
static __device__ __forceinline__ float acc_add_product(float a, float t, float g) {
#pragma clang fp contract(off)
    const float c = t * g;
    return a + c;
}

// division by a workgroup-uniform divisor through its float reciprocal, exact for 0 <= v < 2^24
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
// transposed conv, kernel = stride: one GEMM per kernel tap
//   D[cout, voxel] = sum_cin W_tap[cout, cin] * X[cin, voxel]
// A wave owns 64 input voxels (4 MFMA column blocks) and produces TG taps x NBT cout blocks for them:
// the activation fragments are loaded (and normalised) once and reused for every tap of the group.
// grid.x = N * ceil(vox / 256), grid.y = (taps / TG) * (nblk / NBT).
// ----------------------------------------------------------------------------
template <int NBT, int TG, int MB = 4>                                  // MB: column blocks (16 input voxels each) per wave
__global__ __launch_bounds__(256, 2) void tconv_mfma_kernel(const TconvParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *sSS = (float2 *)smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int vox_in = p.Di * p.Hi * p.Wi;
    constexpr int WGV = 64 * MB;                                          // input voxels per workgroup
    const int wg_per_n = (vox_in + WGV - 1) / WGV;
    const int n = blockIdx.x / wg_per_n;
    const int v0 = (blockIdx.x - n * wg_per_n) * WGV + wave * (16 * MB);
    const int groups = p.nblk / NBT;
    const int tap0 = (blockIdx.y / groups) * TG;
    const int cb0 = (blockIdx.y - (blockIdx.y / groups) * groups) * NBT;

    load_scale_shift(p.src, n, sSS, tid, 256);
    __syncthreads();
    if (v0 >= vox_in && !p.lds_w) return;                              // (with the weights through LDS every wave keeps the k-loop's barriers; its stores are guarded)

    f32x4 acc[MB][TG][NBT];
    const int r = lane & 15, q = lane >> 4;
    // the first k-step starts from the zero constant (no accumulator initialisation), the rest accumulate
    auto kstep = [&](int ks, auto first_c) {
        constexpr bool FIRST = decltype(first_c)::value;
        f16x8 wf[TG][NBT];
#pragma unroll
        for (int tg = 0; tg < TG; ++tg)
#pragma unroll
            for (int nb = 0; nb < NBT; ++nb)
                wf[tg][nb] = *(const f16x8 *)(p.wpk + ((((size_t)(tap0 + tg) * p.nblk + cb0 + nb) * p.ksteps + ks) * 64 + lane) * 8);
        f16x8 xf[MB];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const int v = v0 + mb * 16 + r;
            xf[mb] = load_act_frag(p.src, (size_t)(v < vox_in ? v : vox_in - 1), true, ks * 32 + q * 8, sSS, (size_t)n * vox_in * p.src.C);
        }
#pragma unroll
        for (int tg = 0; tg < TG; ++tg)
#pragma unroll
            for (int nb = 0; nb < NBT; ++nb)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
                    acc[mb][tg][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[tg][nb], xf[mb],
                                          FIRST ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[mb][tg][nb], 0, 0, 0);
    };
    if (!p.lds_w) {
        kstep(0, std::true_type{});
        for (int ks = 1; ks < p.ksteps; ++ks) kstep(ks, std::false_type{});
    } else {
        // Layers with four and more k-steps (>= 128 input channels: the matrix-bound transposed convs in the middle of the decoder): the workgroup's
        // four waves multiply the SAME TG x NBT weight fragments per k-step - each wave loading them from L2 was four times the traffic, and with the
        // activation fragments 96 B per clock and CU against the 64 the L2 delivers (270-280 TFLOP/s whatever the layer).  Here the fragments of
        // k-step ks + 1 are fetched once per workgroup (16 B per thread and 256 fragment elements) while k-step ks multiplies, and go through a
        // double-buffered LDS image; one barrier per k-step.  Same k order, same accumulators: the same bits.
        constexpr int NW = TG * NBT, WPT = (NW * 64 + 255) / 256;           // fragments per k-step; 16-byte elements per thread
        typedef unsigned tc_u32x4 __attribute__((ext_vector_type(4)));
        tc_u32x4 *sWt = (tc_u32x4 *)(smem + (((size_t)p.src.C * 8 + 15) & ~(size_t)15));   // [2][NW][64]
        tc_u32x4 wreg[WPT];
        auto wload = [&](int ks) {
#pragma unroll
            for (int u = 0; u < WPT; ++u) {
                const int e = tid + 256 * u, f = e >> 6, l = e & 63, tg = f / NBT, nb = f - tg * NBT;
                if (NW * 64 % 256 == 0 || e < NW * 64)
                    wreg[u] = *(const tc_u32x4 *)(p.wpk + ((((size_t)(tap0 + tg) * p.nblk + cb0 + nb) * p.ksteps + ks) * 64 + l) * 8);
            }
        };
        auto wstore = [&](int buf) {
#pragma unroll
            for (int u = 0; u < WPT; ++u) {
                const int e = tid + 256 * u;
                if (NW * 64 % 256 == 0 || e < NW * 64) sWt[buf * (NW * 64) + e] = wreg[u];
            }
        };
        auto kstep_l = [&](int ks, auto first_c) {
            constexpr bool FIRST = decltype(first_c)::value;
            if (ks + 1 < p.ksteps) wload(ks + 1);
            f16x8 xf[MB];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const int v = v0 + mb * 16 + r;
                xf[mb] = load_act_frag(p.src, (size_t)(v < vox_in ? v : vox_in - 1), true, ks * 32 + q * 8, sSS, (size_t)n * vox_in * p.src.C);
            }
            const tc_u32x4 *wb = sWt + (ks & 1) * (NW * 64) + lane;
#pragma unroll
            for (int tg = 0; tg < TG; ++tg)
#pragma unroll
                for (int nb = 0; nb < NBT; ++nb) {
                    const f16x8 wf = __builtin_bit_cast(f16x8, wb[(tg * NBT + nb) * 64]);
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
                        acc[mb][tg][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[mb], FIRST ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[mb][tg][nb], 0, 0, 0);
                }
            if (ks + 1 < p.ksteps) wstore((ks + 1) & 1);
            __syncthreads();
        };
        wload(0);
        wstore(0);
        __syncthreads();
        kstep_l(0, std::true_type{});
        for (int ks = 1; ks < p.ksteps; ++ks) kstep_l(ks, std::false_type{});
    }

    const int Ho = p.Hi * p.sh, Wo = p.Wi * p.sw;
    float4 bv[NBT];
#pragma unroll
    for (int nb = 0; nb < NBT; ++nb) bv[nb] = *(const float4 *)(p.bias + (cb0 + nb) * 16 + q * 4);
    const unsigned ovs = (unsigned)FNN_OVS(p);                               // output layout: fnn_device.h, SrcDesc
    const long long ocs = FNN_OCS(p);
    f16 *outi = p.out + (size_t)n * p.Di * p.sd * Ho * Wo * p.Cout;
    // output offsets: a per-voxel base (float-reciprocal division, 24-bit multiplies: input planes < 2^24 voxels, checked
    // by the launcher) plus a wave-uniform offset per tap - the index arithmetic was most of this kernel's instructions
    unsigned toff[TG];
#pragma unroll
    for (int tg = 0; tg < TG; ++tg) {
        const int tap = tap0 + tg;
        const int jd = tap / (p.sh * p.sw), jh = (tap / p.sw) % p.sh, jw = tap % p.sw;     // uniform: scalar unit
        toff[tg] = (unsigned)((jd * Ho + jh) * Wo + jw) * ovs;
    }
    const float rcp_wi = 1.0f / (float)p.Wi, rcp_hi = 1.0f / (float)p.Hi;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int v = v0 + mb * 16 + r;
        if (v >= vox_in) continue;
        const int row = recip_div(v, p.Wi, rcp_wi), iw = v - (int)__umul24(row, p.Wi);
        const int id = recip_div(row, p.Hi, rcp_hi), ih = row - (int)__umul24(id, p.Hi);
        const unsigned ob = ((unsigned)(id * p.sd * Ho + ih * p.sh) * (unsigned)Wo + (unsigned)(iw * p.sw)) * ovs;
        if constexpr (NBT == 2 && TG % 2 == 0) {
            // Taps 2 t, 2 t + 1 are the two w phases of one (d, h) phase (stride 2 along w: the launcher's `row_store`): the
            // 16 input voxels of a column block then make ONE contiguous run of 32 output voxels per cout block.  A second
            // v_permlane16_swap stage sorts the two taps' 16-byte pieces by cout block - lane (r, q) ends with tap q & 1,
            // channel half q >> 1 of voxel r - so that a store instruction writes 1 KB of consecutive bytes (8 whole cache
            // lines) instead of 16 half lines whose other halves arrive with the next instruction (round 4).
            if (p.row_store) {
#pragma unroll
                for (int tg = 0; tg < TG; tg += 2) {
                    fnn_u32x4r pk[2];
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        f16x4 o[2];
#pragma unroll
                        for (int nb = 0; nb < 2; ++nb) {
                            o[nb][0] = (f16)(acc[mb][tg + t][nb][0] + bv[nb].x);
                            o[nb][1] = (f16)(acc[mb][tg + t][nb][1] + bv[nb].y);
                            o[nb][2] = (f16)(acc[mb][tg + t][nb][2] + bv[nb].z);
                            o[nb][3] = (f16)(acc[mb][tg + t][nb][3] + bv[nb].w);
                        }
                        pk[t] = pair_to_b128(o[0], o[1]);                 // lane (r, q): block q & 1, channels 8 (q >> 1) .. of voxel r, tap tg + t
                    }
                    fnn_u32x4r blk[2];
#pragma unroll
                    for (int d = 0; d < 4; ++d) {                        // odd rows of tap 0 <-> even rows of tap 1: [block][lane] with tap = q & 1
                        const auto sw = __builtin_amdgcn_permlane16_swap((unsigned)pk[0][d], (unsigned)pk[1][d], false, false);
                        blk[0][d] = (int)sw[0]; blk[1][d] = (int)sw[1];
                    }
                    const unsigned ov = ob + toff[tg] + (unsigned)(q & 1) * ovs + (unsigned)(q >> 1) * 8u;
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) *(fnn_u32x4r *)(outi + (cb0 + nb) * ocs + ov) = blk[nb];
                }
                continue;
            }
        }
#pragma unroll
        for (int tg = 0; tg < TG; ++tg) {
            const unsigned ov = ob + toff[tg];
            f16x4 o[NBT];
#pragma unroll
            for (int nb = 0; nb < NBT; ++nb) {
                o[nb][0] = (f16)(acc[mb][tg][nb][0] + bv[nb].x);
                o[nb][1] = (f16)(acc[mb][tg][nb][1] + bv[nb].y);
                o[nb][2] = (f16)(acc[mb][tg][nb][2] + bv[nb].z);
                o[nb][3] = (f16)(acc[mb][tg][nb][3] + bv[nb].w);
            }
            if constexpr (NBT == 2) {
                // the two cout blocks of a voxel as ONE 16-byte store per lane (pair_to_b128: lane (r, q) then holds channels
                // 8 (q >> 1) .. + 7 of block q & 1): 64 contiguous bytes per voxel and instruction instead of 2 x 32
                *(fnn_u32x4r *)(outi + (cb0 + (q & 1)) * ocs + ov + (q >> 1) * 8) = pair_to_b128(o[0], o[1]);
            } else {
                *(f16x4 *)(outi + cb0 * ocs + ov + q * 4) = o[0];
            }
        }
    }
}

void tconv_pack_weights(const float *W, int cin, int cout, int cout_pad, int taps, int ksteps, unsigned short *dst) {
    const int nblk = cout_pad / 16;
    for (int tap = 0; tap < taps; ++tap)
        for (int cb = 0; cb < nblk; ++cb)
            for (int ks = 0; ks < ksteps; ++ks)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int ci = ks * 32 + 8 * (lane >> 4) + j, co = cb * 16 + (lane & 15);
                        float v = 0.f;
                        if (ci < cin && co < cout) v = W[((size_t)ci * cout + co) * taps + tap];
                        dst[((((size_t)tap * nblk + cb) * ksteps + ks) * 64 + lane) * 8 + j] = fnn_half_bits(v);
                    }
}

int launch_tconv(const TconvParams &p, hipStream_t st) {
    const int vox_in = p.Di * p.Hi * p.Wi;
    if ((long long)p.Di * p.Hi * p.Wi > (1 << 24)) return -1;       // the kernel's float-reciprocal index arithmetic
    const int taps = p.sd * p.sh * p.sw;
    size_t lds = (size_t)p.src.C * 8;
    // accumulators: 4 column blocks x TG taps x NBT cout blocks x 4 registers; keep TG * NBT <= 4
    const int nbt = (p.nblk % 2 == 0) ? 2 : 1;
    // two cout blocks x 4 taps held 128 accumulator registers (276 VGPRs: one wave per SIMD); two taps: 152, three waves
    // per SIMD, the activations are read once more - 6 % less tconv time on the benchmark net
    // (round 2, late: with the 16-byte stores four taps per wave win - 9.3 -> 7.9 ms per volume; eight taps on two column
    // blocks per wave - every activation read once - measured the same as four: not kept)
    if (taps < 2) return -1;                                           // kernel = stride (1, 1, 1) is not a transposed conv of a U-Net decoder
    static const int tg_max2 = fnn_knob("FNN_TCONV_TG") && atoi(fnn_knob("FNN_TCONV_TG")) == 2 ? 2 : 4;       // A-B aid
    const int tg_cap = nbt == 2 ? tg_max2 : 4;
    const int tg = taps >= tg_cap ? tg_cap : taps;                     // taps is 2, 4 or 8
    dim3 grid(p.N * ((vox_in + 255) / 256), (taps / tg) * (p.nblk / nbt));
    TconvParams pp = p;
    // whole-row stores (see the kernel): the taps of a workgroup come in pairs that differ in the w phase only.  Measured
    // (FNN_TCONV_NO_ROWSTORE: A-B aid): transposed convs 8.1 -> 7.7 ms per benchmark volume, teacher 26.7 -> 25.6; two column
    // blocks per wave at four waves per SIMD (98 registers) next to it: 8.35 - dropped
    pp.row_store = p.sw == 2 && nbt == 2 && tg % 2 == 0 && fnn_knob("FNN_TCONV_NO_ROWSTORE") == nullptr;
    pp.lds_w = p.ksteps >= 4 && fnn_knob("FNN_TCONV_NO_LDSW") == nullptr;      // (knob: A-B aid) the weight fragments once per workgroup through LDS
    if (pp.lds_w) lds = ((lds + 15) & ~(size_t)15) + (size_t)2 * tg * nbt * 1024;
#define FNN_TCONV(NBTv, TGv) do { fnn_note_kernel("tconv_mfma_kernel<%d,%d>", NBTv, TGv); hipLaunchKernelGGL((tconv_mfma_kernel<NBTv, TGv>), grid, dim3(256), lds, st, pp); } while (0)
    if (nbt == 2) { if (tg == 4) FNN_TCONV(2, 4); else FNN_TCONV(2, 2); }
    else          { if (tg == 4) FNN_TCONV(1, 4); else FNN_TCONV(1, 2); }
#undef FNN_TCONV
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ----------------------------------------------------------------------------
// volume accumulators
// ----------------------------------------------------------------------------
// Layout: acc[AX][Y][Z][HP], channels-last, fp16 (reference rounding) or fp32;
//   channel h < heads      sum over patches of  gaussian * logit_h
//   channel heads          sum of the gaussian weights (the reference's n_predictions)
//   HP = round_up(heads + 1, 8) so that 4 consecutive channels are an aligned 8 / 16 bytes.
// One voxel's channels are one or two contiguous 128-byte lines: a patch touches ~5x fewer pages
// than with a [heads][X][Y][Z] layout, the MFMA result (4 consecutive heads of one voxel per lane)
// is added straight from registers, and divide / argmax read one line per voxel.
//
// Reference rounding (predict_from_raw_data.py:611-614):
//   pred (fp32) *= gaussian (fp16)      -> fp32 product           (__fmul_rn: never fused)
//   acc (fp16)[sl] += pred              -> fp32 add, ONE round-to-nearest-even to fp16
//   n   (fp16)[sl] += gaussian          -> fp16 + fp16
// fp16 subnormals must survive (5.96e-8 weights): no flush-to-zero is used.
template <bool ACC32>
static __device__ __forceinline__ void acc_add4(void *acc, size_t elem, const float c[4], unsigned mask) {
    if (ACC32) {
        f32x4 *ap = (f32x4 *)((float *)acc + elem);
        f32x4 a = *ap;
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = (mask >> j) & 1 ? __fadd_rn(a[j], c[j]) : a[j];
        *ap = a;
    } else {
        f16x4 *ap = (f16x4 *)((f16 *)acc + elem);
        f16x4 a = *ap;
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = (mask >> j) & 1 ? (f16)__fadd_rn((float)a[j], c[j]) : a[j];
        *ap = a;
    }
}

// ----------------------------------------------------------------------------
// seg head for the mirroring path / raw patch logits:
//   D[head, voxel] = Wseg[head, c] * act[c, voxel] + bias -> patch_buf[head][unflip(voxel)] (=, +=)
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_head_kernel(const HeadParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float2 *sSS = (float2 *)smem;
    float *sT = (float *)(smem + ((p.src.C * 8 + 255) & ~255)) + wave * (64 * 65);   // [64 heads][64(+1) voxels]
    const int P = p.PD * p.PH * p.PW;

    load_scale_shift(p.src, p.b, sSS, tid, 256);
    __syncthreads();

    const int v0 = (blockIdx.x * 4 + wave) * 64;
    if (v0 >= P) return;
    const int r = lane & 15, q = lane >> 4;
    const int v = v0 + lane;
    const bool vok = v < P;
    int w = v % p.PW, h = (v / p.PW) % p.PH, d = v / (p.PW * p.PH);
    if (p.flip_d) d = p.PD - 1 - d;
    if (p.flip_h) h = p.PH - 1 - h;
    if (p.flip_w) w = p.PW - 1 - w;
    const int pv = (d * p.PH + h) * p.PW + w;                 // voxel index in patch space

    for (int hb0 = 0; hb0 < p.hblocks; hb0 += 4) {
        const int nhb = min(4, p.hblocks - hb0);
        // the accumulators start from the bias (the MFMA's C operand: no add behind it) - in every seg-head kernel and
        // in gather_head_kernel alike, whose logits must agree bit for bit
        f32x4 acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const f32x4 b4 = a < nhb ? *(const f32x4 *)(p.bias + (hb0 + a) * 16 + q * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = b4;
        }
        for (int ks = 0; ks < p.ksteps; ++ks) {
            f16x8 xf[4];
#pragma unroll
            for (int vb = 0; vb < 4; ++vb) {
                const int vv = v0 + vb * 16 + r;
                xf[vb] = load_act_frag(p.src, (size_t)p.b * P + vv, vv < P, ks * 32 + q * 8, sSS);
            }
#pragma unroll
            for (int hb = 0; hb < 4; ++hb) {
                if (hb < nhb) {
                    const f16x8 wf = *(const f16x8 *)(p.wpk + (((size_t)(hb0 + hb) * p.ksteps + ks) * 64 + lane) * 8);
#pragma unroll
                    for (int vb = 0; vb < 4; ++vb)
                        acc[hb][vb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[vb], acc[hb][vb], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int hb = 0; hb < 4; ++hb)
#pragma unroll
            for (int vb = 0; vb < 4; ++vb)
#pragma unroll
                for (int j = 0; j < 4; ++j) sT[(hb * 16 + q * 4 + j) * 65 + vb * 16 + r] = acc[hb][vb][j];
        __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0): this wave's LDS writes landed
        __builtin_amdgcn_wave_barrier();
        if (vok) {
            const int nh = min(64, p.heads - hb0 * 16);
            for (int hl = 0; hl < nh; ++hl) {
                const int head = hb0 * 16 + hl;
                const float val = sT[hl * 65 + lane];
                float *pb = p.patch_buf + (size_t)head * P + pv;
                *pb = (p.mode == 1) ? val : (*pb + val);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ----------------------------------------------------------------------------
// fused seg head + Gaussian weighting + accumulate (no mirroring): the K6 + K7 kernel
// ----------------------------------------------------------------------------
// One wave = 64 consecutive patch voxels, processed as two rounds of 32.  Per round the MFMA result
// (4 consecutive heads of one voxel per lane) is transposed through LDS so that 8 lanes own the 8
// channel groups of ONE voxel: every wave instruction of the read-modify-write then covers 8 whole
// accumulator lines (rocprof showed 1.75x write amplification when lanes wrote 32-byte pieces of a
// line straight from the MFMA registers).  The 4 accumulator loads of a round are issued before its
// MFMAs, so a round costs one global round trip.
#define HEAD_LD 68                        // LDS row stride in floats (64 channels + pad, 16-B aligned rows)
template <bool ACC32>
__global__ __launch_bounds__(256) void seg_head_acc_kernel(const HeadParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float2 *sSS = (float2 *)smem;
    float *sT = (float *)(smem + ((p.src.C * 8 + 255) & ~255)) + wave * (32 * HEAD_LD);      // [32 voxels][64 ch]
    const int P = p.PD * p.PH * p.PW;
    load_scale_shift(p.src, p.b, sSS, tid, 256);
    __syncthreads();

    const int v0 = (blockIdx.x * 4 + wave) * 64;
    if (v0 >= P) return;
    const int r = lane & 15, q = lane >> 4;
    const int grp = lane & 7, vsub = lane >> 3;              // read-modify-write role: channel group, voxel in round

    // All global loads of a round are issued unconditionally (clamped addresses) and back to back, so a
    // round costs ONE memory round trip; predicates are applied to the values afterwards.  (With per-lane
    // `if`s around the loads hipcc serialised them behind s_waitcnt vmcnt(0): ~12 round trips per round.)
    for (int cb0 = 0; cb0 < p.HP; cb0 += 64) {               // 64 accumulator channels at a time
        const int hb_first = cb0 >> 4;
        const int grp_c = cb0 + grp * 8 < p.HP ? grp : 0;     // clamp: lanes past HP re-read group 0 and write nothing
        const bool grp_ok = cb0 + grp * 8 < p.HP;
        // bias of this lane's 4 channels per head block (the bias array is zero padded to hblocks * 16)
        f32x4 bv[4];
#pragma unroll
        for (int hb = 0; hb < 4; ++hb) {
            const int hbc = hb_first + hb < p.hblocks ? hb_first + hb : p.hblocks - 1;
            bv[hb] = *(const f32x4 *)(p.bias + hbc * 16 + q * 4);
        }
#pragma unroll 1
        for (int rd = 0; rd < 2; ++rd) {
            size_t aelem[4];
            float g[4];
            bool ok[4];
            f16x8 a16[4];
            f32x4 a32[4][2];
            f16 graw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int v = v0 + rd * 32 + 8 * i + vsub;
                ok[i] = v < P && grp_ok;
                const int vv = v < P ? v : P - 1;
                const int w = vv % p.PW, h = (vv / p.PW) % p.PH, d = vv / (p.PW * p.PH);
                aelem[i] = (((size_t)(p.ox + d) * p.Y + (p.oy + h)) * p.Z + (p.oz + w)) * p.HP + cb0 + grp_c * 8;
                graw[i] = p.gauss ? p.gauss[vv] : (f16)1.f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (ACC32) { a32[i][0] = *(const f32x4 *)((const float *)p.acc + aelem[i]); a32[i][1] = *(const f32x4 *)((const float *)p.acc + aelem[i] + 4); }
                else a16[i] = *(const f16x8 *)((const f16 *)p.acc + aelem[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = (float)graw[i];

            // MFMA: [heads of this 64-channel block] x [32 voxels]
            f32x4 acc[4][2];
#pragma unroll
            for (int hb = 0; hb < 4; ++hb)
#pragma unroll
                for (int vb = 0; vb < 2; ++vb) acc[hb][vb] = bv[hb];    // bias = the MFMA's C operand (as in every head kernel)
            for (int ks = 0; ks < p.ksteps; ++ks) {
                f16x8 xf[2], wf[4];
#pragma unroll
                for (int hb = 0; hb < 4; ++hb) {
                    const int hbc = hb_first + hb < p.hblocks ? hb_first + hb : p.hblocks - 1;
                    wf[hb] = *(const f16x8 *)(p.wpk + (((size_t)hbc * p.ksteps + ks) * 64 + lane) * 8);
                }
#pragma unroll
                for (int vb = 0; vb < 2; ++vb) {
                    const int v = v0 + (rd * 2 + vb) * 16 + r;
                    xf[vb] = load_act_frag(p.src, (size_t)p.b * P + (v < P ? v : P - 1), true, ks * 32 + q * 8, sSS);
                }
#pragma unroll
                for (int hb = 0; hb < 4; ++hb)
#pragma unroll
                    for (int vb = 0; vb < 2; ++vb)
                        acc[hb][vb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[hb], xf[vb], acc[hb][vb], 0, 0, 0);
            }
            // logits (+ bias) -> LDS, [voxel][channel]
#pragma unroll
            for (int hb = 0; hb < 4; ++hb)
#pragma unroll
                for (int vb = 0; vb < 2; ++vb) {
                    const f32x4 t = hb_first + hb < p.hblocks ? acc[hb][vb] : (f32x4){0.f, 0.f, 0.f, 0.f};
                    *(f32x4 *)(sT + (vb * 16 + r) * HEAD_LD + hb * 16 + q * 4) = t;
                }
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
            // read-modify-write: 8 lanes x 16 B (fp16) cover one voxel's 64 channels
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 t0 = *(const f32x4 *)(sT + (8 * i + vsub) * HEAD_LD + grp_c * 8);
                const f32x4 t1 = *(const f32x4 *)(sT + (8 * i + vsub) * HEAD_LD + grp_c * 8 + 4);
                float c[8];
                unsigned mask = 0;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int ch = cb0 + grp_c * 8 + e;
                    const float t = e < 4 ? t0[e] : t1[e - 4];
                    c[e] = ch == p.heads ? g[i] : __fmul_rn(t, g[i]);      // channel `heads` accumulates the weight
                    if (ch <= p.heads) mask |= 1u << e;                      // padding channels keep their bits
                }
                if (ACC32) {
                    f32x4 b0 = a32[i][0], b1 = a32[i][1];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        b0[e] = (mask >> e) & 1 ? __fadd_rn(b0[e], c[e]) : b0[e];
                        b1[e] = (mask >> (4 + e)) & 1 ? __fadd_rn(b1[e], c[4 + e]) : b1[e];
                    }
                    if (ok[i]) {
                        *(f32x4 *)((float *)p.acc + aelem[i]) = b0;
                        *(f32x4 *)((float *)p.acc + aelem[i] + 4) = b1;
                    }
                } else {
                    f16x8 bq = a16[i];
#pragma unroll
                    for (int e = 0; e < 8; ++e) bq[e] = (mask >> e) & 1 ? (f16)__fadd_rn((float)bq[e], c[e]) : bq[e];
                    if (ok[i]) *(f16x8 *)((f16 *)p.acc + aelem[i]) = bq;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// One-k-step (C <= 32) version of seg_head_acc_kernel with every global load of BOTH rounds issued up front.
// vmcnt retires in order, so a load issued after a store cannot be consumed before that store has been
// acknowledged: with the loads of round 1 behind the stores of round 0 (the loop above), every wave waited for a
// full write round trip in the middle of its life.  Here the only waits are for loads that were issued before any
// store; the stores of both rounds drain while the wave finishes.
template <bool ACC32, int RD, int NT = 0, int MINB = 1>
__global__ __launch_bounds__(256, MINB) void seg_head_acc1_kernel(const HeadParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float2 *sSS = (float2 *)smem;
    float *sT = (float *)(smem + ((p.src.C * 8 + 255) & ~255)) + wave * (32 * HEAD_LD);      // [32 voxels][64 ch]
    const int P = p.PD * p.PH * p.PW;
    load_scale_shift(p.src, p.b, sSS, tid, 256);
    __syncthreads();

    const int v0 = (blockIdx.x * 4 + wave) * (32 * RD);
    if (v0 >= P) return;
    const int r = lane & 15, q = lane >> 4;
    const int grp = lane & 7, vsub = lane >> 3;
    const float rcp_pw = 1.0f / (float)p.PW, rcp_ph = 1.0f / (float)p.PH;

    for (int cb0 = 0; cb0 < p.HP; cb0 += 64) {
        const int hb_first = cb0 >> 4;
        const int grp_c = cb0 + grp * 8 < p.HP ? grp : 0;
        const bool grp_ok = cb0 + grp * 8 < p.HP;
        // ---- phase A: every address, then every load (accumulator lines, Gaussian weights, activation fragments)
        size_t aelem[RD][4];
        bool ok[RD][4], first[RD][4];
        f16 graw[RD][4];
        f16x8 a16[RD][4];
        f32x4 a32[ACC32 ? RD : 1][4][2];
        f16x8 xraw[RD][2];
#pragma unroll
        for (int rd = 0; rd < RD; ++rd)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int v = v0 + rd * 32 + 8 * i + vsub;
                ok[rd][i] = v < P && grp_ok;
                const int vv = v < P ? v : P - 1;
                // float-reciprocal division (P <= 2^24, checked by the launcher): three 32-bit integer divisions per voxel
                // were a fifth of this kernel's instructions
                const int row = recip_div(vv, p.PW, rcp_pw), w = vv - row * p.PW;
                const int d = recip_div(row, p.PH, rcp_ph), h = row - d * p.PH;
                aelem[rd][i] = (((size_t)(p.ox + d) * p.Y + (p.oy + h)) * p.Z + (p.oz + w)) * p.HP + cb0 + grp_c * 8;
                first[rd][i] = d >= p.fx && h >= p.fy && w >= p.fz;     // nobody has written this voxel yet
                graw[rd][i] = p.gauss[vv];                              // always a map (all ones without Gaussian weighting)
            }
        // first-visit voxels read one (hot) line of the patch's first voxel instead of their own: the load stays
        // unconditional (lesson 1 in DESIGN.md) and costs no HBM traffic; its value is discarded below
        const size_t dummy = (((size_t)p.ox * p.Y + p.oy) * p.Z + p.oz) * p.HP + cb0 + grp_c * 8;
#pragma unroll
        for (int rd = 0; rd < RD; ++rd)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t le = first[rd][i] ? dummy : aelem[rd][i];
                if (ACC32) {
                    a32[ACC32 ? rd : 0][i][0] = *(const f32x4 *)((const float *)p.acc + le);
                    a32[ACC32 ? rd : 0][i][1] = *(const f32x4 *)((const float *)p.acc + le + 4);
                } else if (NT & 2) a16[rd][i] = __builtin_nontemporal_load((const f16x8 *)((const f16 *)p.acc + le));
                else a16[rd][i] = *(const f16x8 *)((const f16 *)p.acc + le);
            }
        const int c0 = q * 8 < p.src.C ? q * 8 : 0;
#pragma unroll
        for (int rd = 0; rd < RD; ++rd)
#pragma unroll
            for (int vb = 0; vb < 2; ++vb) {
                const int v = v0 + (rd * 2 + vb) * 16 + r;
                xraw[rd][vb] = *(const f16x8 *)(p.src.ptr + ((size_t)p.b * P + (v < P ? v : P - 1)) * p.src.C + c0);
            }
        f16x8 wf[4];
        f32x4 bv[4];
#pragma unroll
        for (int hb = 0; hb < 4; ++hb) {
            const int hbc = hb_first + hb < p.hblocks ? hb_first + hb : p.hblocks - 1;
            wf[hb] = *(const f16x8 *)(p.wpk + ((size_t)hbc * 64 + lane) * 8);
            bv[hb] = *(const f32x4 *)(p.bias + hbc * 16 + q * 4);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- phase B: per round MFMA -> LDS transpose -> read-modify-write -> store
#pragma unroll
        for (int rd = 0; rd < RD; ++rd) {
            f32x4 acc[4][2];
#pragma unroll
            for (int vb = 0; vb < 2; ++vb) {
                const f16x8 xf = norm_act_frag(p.src, xraw[rd][vb], q * 8, sSS);
#pragma unroll
                for (int hb = 0; hb < 4; ++hb)
                    acc[hb][vb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[hb], xf, bv[hb], 0, 0, 0);       // bias = C operand
            }
#pragma unroll
            for (int hb = 0; hb < 4; ++hb)
#pragma unroll
                for (int vb = 0; vb < 2; ++vb) {
                    const f32x4 t = hb_first + hb < p.hblocks ? acc[hb][vb] : (f32x4){0.f, 0.f, 0.f, 0.f};
                    *(f32x4 *)(sT + (vb * 16 + r) * HEAD_LD + hb * 16 + q * 4) = t;
                }
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 t0 = *(const f32x4 *)(sT + (8 * i + vsub) * HEAD_LD + grp_c * 8);
                const f32x4 t1 = *(const f32x4 *)(sT + (8 * i + vsub) * HEAD_LD + grp_c * 8 + 4);
                // No per-channel cases: channel `heads` (the weight sum) has zero weights and bias 1 (fnn_load_weights), so
                // its product is 1 * g = g; padding channels have zero weights and bias and add 0.
                const float g = (float)graw[rd][i];
                if (ACC32) {
                    f32x4 b0 = a32[ACC32 ? rd : 0][i][0], b1 = a32[ACC32 ? rd : 0][i][1];
                    if (first[rd][i]) { b0 = (f32x4){0.f, 0.f, 0.f, 0.f}; b1 = b0; }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        b0[e] = acc_add_product(b0[e], t0[e], g);
                        b1[e] = acc_add_product(b1[e], t1[e], g);
                    }
                    if (ok[rd][i]) {
                        *(f32x4 *)((float *)p.acc + aelem[rd][i]) = b0;
                        *(f32x4 *)((float *)p.acc + aelem[rd][i] + 4) = b1;
                    }
                } else {
                    f16x8 bq = a16[rd][i];
                    if (first[rd][i]) bq = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};      // 0 + c, like the zero-filled accumulator
#pragma unroll
                    for (int e = 0; e < 8; ++e) bq[e] = (f16)acc_add_product((float)bq[e], e < 4 ? t0[e] : t1[e - 4], g);
                    if (ok[rd][i]) {
                        if (NT & 1) __builtin_nontemporal_store(bq, (f16x8 *)((f16 *)p.acc + aelem[rd][i]));
                        else *(f16x8 *)((f16 *)p.acc + aelem[rd][i]) = bq;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// Only the vectorised accumulate kernel knows the first-visit thresholds (one k-step: <= 32 input channels).
bool launch_head_first_visit_ok(const HeadParams &p) {
    static const bool head_v1 = fnn_knob("FNN_HEAD_V1") != nullptr;
    return p.mode == 0 && p.ksteps == 1 && !head_v1 && (long long)p.PD * p.PH * p.PW <= (1 << 24);
}

int launch_head(const HeadParams &p, hipStream_t st) {
    const int P = p.PD * p.PH * p.PW;
    fnn_allow_lds<seg_head_kernel>();
    dim3 grid((P + 255) / 256);
    if (p.mode == 0) {
        const size_t lds = (size_t)((p.src.C * 8 + 255) & ~255) + (size_t)4 * 32 * HEAD_LD * 4;
        static const bool head_v1 = fnn_knob("FNN_HEAD_V1") != nullptr;            // A-B aid
        if (p.ksteps == 1 && !head_v1 && P <= (1 << 24)) {
            // two 32-voxel rounds per wave (one: faster alone, slower next to the other stream); fp16 buffers: non-temporal
            // accumulator traffic (each line is touched once per patch: +1.3 % on the round-1 benchmark) and registers for two
            // workgroups per SIMD (177 VGPRs instead of 214).  The A-B variants of those choices (FNN_HEAD_RD / _NT / _MINB)
            // were six more kernels that nothing but a knob selected: gone (round 3).
            fnn_note_kernel(p.acc_fp32 ? "seg_head_acc1_kernel<1,2>" : "seg_head_acc1_kernel<0,2,3,2>");
            if (p.acc_fp32) hipLaunchKernelGGL((seg_head_acc1_kernel<true, 2>), grid, dim3(256), lds, st, p);
            else hipLaunchKernelGGL((seg_head_acc1_kernel<false, 2, 3, 2>), grid, dim3(256), lds, st, p);
        } else {
            fnn_note_kernel("seg_head_acc_kernel<%d>", p.acc_fp32 ? 1 : 0);
            if (p.acc_fp32) hipLaunchKernelGGL(seg_head_acc_kernel<true>, grid, dim3(256), lds, st, p);
            else hipLaunchKernelGGL(seg_head_acc_kernel<false>, grid, dim3(256), lds, st, p);
        }
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    const size_t lds = (size_t)((p.src.C * 8 + 255) & ~255) + (size_t)4 * 64 * 65 * 4;
    fnn_note_kernel("seg_head_kernel");
    return fnn_launch_lds<seg_head_kernel>(grid, dim3(256), lds, st, p);
}

// ----------------------------------------------------------------------------
// mirrored evaluations: mean of the patch buffer -> accumulators
// (predict_from_raw_data.py:556 `prediction /= n`, then :611-614)
// One thread = one voxel x 4 channels.
// ----------------------------------------------------------------------------
template <bool ACC32>
__global__ __launch_bounds__(256) void patch_acc_kernel(const PatchAccParams p) {
    const int P = p.PD * p.PH * p.PW;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= P) return;
    const int w = v % p.PW, h = (v / p.PW) % p.PH, d = v / (p.PW * p.PH);
    const float g = p.gauss ? (float)p.gauss[v] : 1.f;
    const size_t aelem = (((size_t)(p.ox + d) * p.Y + (p.oy + h)) * p.Z + (p.oz + w)) * p.HP;
    const float div = (float)p.n_div;
    for (int ch0 = 0; ch0 <= p.heads; ch0 += 4) {
        float c[4];
        unsigned mask = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = ch0 + j;
            c[j] = 0.f;
            if (ch < p.heads) { c[j] = __fmul_rn(__fdiv_rn(p.patch_buf[(size_t)ch * P + v], div), g); mask |= 1u << j; }
            else if (ch == p.heads) { c[j] = g; mask |= 1u << j; }
        }
        acc_add4<ACC32>(p.acc, aelem + ch0, c, mask);
    }
}

int launch_patch_acc(const PatchAccParams &p, hipStream_t st) {
    const int P = p.PD * p.PH * p.PW;
    fnn_note_kernel("patch_acc_kernel<%d>", p.acc_fp32 ? 1 : 0);
    if (p.acc_fp32) hipLaunchKernelGGL(patch_acc_kernel<true>, dim3((P + 255) / 256), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(patch_acc_kernel<false>, dim3((P + 255) / 256), dim3(256), 0, st, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

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
    const size_t aelem = (((size_t)(x + p.lo_x) * p.Y + (y + p.lo_y)) * p.Z + (z + p.lo_z)) * p.HP;
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
    const AT *src = (const AT *)p.acc + (((size_t)(x + p.lo_x) * p.Y + (y + p.lo_y)) * p.Z + (z0 + p.lo_z)) * HP;
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

// Label map straight from the accumulators: argmax_h(acc_h / wsum) with the reference's rounding
// (divide, round to fp16, first maximum wins) without materialising the logits.
// LabelManager.convert_logits_to_segmentation on one voxel's logits (label_handling.py:163-181):
//   plain labels: numpy argmax - first maximum wins, the first NaN wins;
//   regions     : label 0, then for i in order: if sigmoid(float(logit_i)) > 0.5: label = regions_class_order[i].
// torch's fp32 sigmoid exceeds 0.5 exactly for x > 1.5 * 2^-24 (probed over every fp32 around the threshold and every
// fp16 value, tests/test_oracle_golden.py) - "logit > 0" would differ for the two smallest positive fp16 values.
#define FNN_SIGMOID_HALF_THRESHOLD 0x1.8p-24f
struct LabelPick {
    float best = 0.f; int arg = 0; bool best_nan = false; int seg = 0;
    __device__ __forceinline__ void feed(int h, float v, const int *order) {
        if (order) { if (v > FNN_SIGMOID_HALF_THRESHOLD) seg = order[h]; }
        else if (h == 0) { best = v; best_nan = v != v; }
        else if (!best_nan && (v > best || v != v)) { best = v; arg = h; best_nan = v != v; }
    }
    __device__ __forceinline__ int result(const int *order) const { return order ? seg : arg; }
};

template <bool ACC32, typename LT>
__global__ __launch_bounds__(256) void labels_from_acc_kernel(const FinalizeParams p, LT *labels, const int *order) {
    const long long nbox = p.OX * p.OY * p.OZ;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nbox) return;
    const long long z = i % p.OZ, y = (i / p.OZ) % p.OY, x = i / (p.OZ * p.OY);
    const size_t aelem = (((size_t)(x + p.lo_x) * p.Y + (y + p.lo_y)) * p.Z + (z + p.lo_z)) * p.HP;
    const size_t oidx0 = ((size_t)(x + p.out_x) * p.out_Y + (y + p.out_y)) * p.out_Z + (z + p.out_z);
    const float wsum = ACC32 ? ((const float *)p.acc)[aelem + p.heads] : (float)((const f16 *)p.acc)[aelem + p.heads];
    LabelPick pick;
    bool bad = false;
    for (int h = 0; h < p.heads; ++h) {
        const float a = ACC32 ? ((const float *)p.acc)[aelem + h] : (float)((const f16 *)p.acc)[aelem + h];
        const float v = (float)(f16)__fdiv_rn(a, wsum);
        bad |= isinf(v);
        pick.feed(h, v, order);
    }
    labels[oidx0] = (LT)pick.result(order);
    if (bad) atomicOr(p.inf_flag, 1);
}

// The same with G = 2^LOG_G consecutive lanes per voxel, each lane on 8 channels (one 16-byte piece of an fp16
// accumulator line, two of an fp32 one): a wave instruction then reads 64 / G whole voxel lines - contiguous along z -
// instead of 2 bytes out of 64 different lines, 61 times over (the one-thread-per-voxel form above re-fetched every
// line many times: 75 ms for the 17 GB of a 512^3 x 61 volume, this one runs at the HBM rate).  The lanes' partial
// results are merged in channel order, so "first maximum / first NaN wins" and "last region above the threshold
// wins" are exactly the sequential rule.
template <bool ACC32, typename LT, int LOG_G>
__global__ __launch_bounds__(256) void labels_from_acc_coop_kernel(const FinalizeParams p, LT *labels, const int *order) {
    constexpr int G = 1 << LOG_G;
    const long long nbox = p.OX * p.OY * p.OZ;
    const long long gt = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long iv = gt >> LOG_G;
    const int piece = (int)(gt & (G - 1));
    const long long i = iv < nbox ? iv : nbox - 1;                   // surplus lanes redo the last voxel (no store)
    const long long z = i % p.OZ, y = (i / p.OZ) % p.OY, x = i / (p.OZ * p.OY);
    const size_t aelem = (((size_t)(x + p.lo_x) * p.Y + (y + p.lo_y)) * p.Z + (z + p.lo_z)) * p.HP;
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
    // local pick over this lane's channels (in order)
    float best = 0.f; int arg = -1; bool nan = false; int hit = -1; bool bad = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int h = c0 + j;
        if (h < p.heads) {
            const float q = (float)(f16)__fdiv_rn(v[j], wsum);
            bad |= isinf(q);
            if (q > FNN_SIGMOID_HALF_THRESHOLD) hit = h;
            if (arg < 0) { best = q; arg = h; nan = q != q; }
            else if (!nan && (q > best || q != q)) { best = q; arg = h; nan = q != q; }
        }
    }
    // merge in channel order: the lower lane holds the lower channels
#pragma unroll
    for (int m = 1; m < G; m <<= 1) {
        const float ob = __shfl_xor(best, m, 64);
        const int oa = __shfl_xor(arg, m, 64), on = __shfl_xor((int)nan, m, 64), oh = __shfl_xor(hit, m, 64);
        const bool lower = (piece & m) == 0;
        // (lo, hi) = (mine, other) when this lane is the lower one
        const float lb = lower ? best : ob, hb = lower ? ob : best;
        const int la = lower ? arg : oa, ha = lower ? oa : arg;
        const bool ln = lower ? nan : (on != 0), hn = lower ? (on != 0) : nan;
        bool take_hi;
        if (la < 0) take_hi = true;                                   // the lower part holds no head
        else if (ha < 0) take_hi = false;
        else if (ln) take_hi = false;
        else take_hi = hn || hb > lb;
        best = take_hi ? hb : lb; arg = take_hi ? ha : la; nan = take_hi ? hn : ln;
        hit = hit > oh ? hit : oh;
    }
    if (piece == 0 && iv < nbox) {
        const size_t oidx0 = ((size_t)(x + p.out_x) * p.out_Y + (y + p.out_y)) * p.out_Z + (z + p.out_z);
        labels[oidx0] = (LT)(order ? (hit >= 0 ? order[hit] : 0) : arg);
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
// logits [heads][n_vox] -> label map (argmax or regions, see LabelPick)
// ----------------------------------------------------------------------------
template <typename LT>
__global__ __launch_bounds__(256) void argmax_kernel(const void *logits, int fp32, int heads, long long nvox, LT *labels,
                                                     const int *order) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvox) return;
    LabelPick pick;
    for (int h = 0; h < heads; ++h) {
        const float v = fp32 ? ((const float *)logits)[(size_t)h * nvox + i] : (float)((const f16 *)logits)[(size_t)h * nvox + i];
        pick.feed(h, v, order);
    }
    labels[i] = (LT)pick.result(order);
}

int launch_argmax(const void *logits, int fp32, int heads, long long nvox, void *labels, int label_u16, const int *order,
                  hipStream_t st) {
    const dim3 grid((unsigned)((nvox + 255) / 256));
    if (label_u16) hipLaunchKernelGGL(argmax_kernel<uint16_t>, grid, dim3(256), 0, st, logits, fp32, heads, nvox, (uint16_t *)labels, order);
    else hipLaunchKernelGGL(argmax_kernel<uint8_t>, grid, dim3(256), 0, st, logits, fp32, heads, nvox, (uint8_t *)labels, order);
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

