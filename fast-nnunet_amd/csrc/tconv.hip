// tconv.hip - ConvTranspose3d(kernel = stride) on the matrix cores (gfx950)
#include "act_load.h"
#include <cstdlib>
#include <type_traits>

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
