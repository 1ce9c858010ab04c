// conv3d.hip - Conv3d for gfx950 (MI355X): the K1 kernels of SURVEY.md 2.3.
//
//   conv3d_mfma_kernel   generic implicit-GEMM conv on the matrix cores
//                        (v_mfma_f32_16x16x32_f16), any per-axis kernel 1|3 and
//                        stride 1|2, one or two channels-last inputs (the second
//                        input replaces torch.cat((up, skip), 1)), InstanceNorm +
//                        LeakyReLU of the producer applied while staging, the
//                        InstanceNorm statistics of THIS conv accumulated in the
//                        epilogue.
//   (the first conv of the network, 1..8 input channels read straight out of
//    the fp32 volume, lives in stem.hip)
//
// Replaces torch.nn.Conv3d + InstanceNorm3d + LeakyReLU as composed by
// dynamic_network_architectures' ConvDropoutNormReLU, which the reference
// instantiates at nnUNetDistillationTrainer.py:141-173.
#include "fnn_device.h"
#include "conv_common.h"
#include <cstdlib>

// ----------------------------------------------------------------------------
// generic MFMA conv
// ----------------------------------------------------------------------------
// GEMM view per workgroup:  D[cout, voxel] = sum_k W[cout, k] * X[k, voxel]
//   voxel : a 4 x 8 x 8 output tile (256 voxels); wave w owns depth slice w,
//           its 4 MFMA column blocks are pairs of rows (16 voxels each);
//   k     : input channels in chunks of 16; one k-step (32) = 2 taps x 16 ch;
//   cout  : NB blocks of 16 per workgroup (blockIdx.y picks the group).
// Weights are the MFMA "A" operand so that each lane ends up with 4
// consecutive output channels of one voxel: an 8-byte channels-last store.
//
// LDS: [halo tile of the current 16-channel chunk : voxels x 32 B]
//      [weight fragments of the chunk : ksteps x NB x 1 KiB]
//      [global offsets of the halo voxels : int per voxel]
//      [per-input-channel (scale, shift)] [tap offsets]
template <int NB>
__global__ __launch_bounds__(256) void conv3d_mfma_kernel(const ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    int t = blockIdx.x;
    const int tw = t % p.tiles_w; t /= p.tiles_w;
    const int th = t % p.tiles_h; t /= p.tiles_h;
    const int td = t % p.tiles_d;
    const int n = t / p.tiles_d;
    const int cb0 = blockIdx.y * NB;

    const int od0 = td * FNN_TILE_D, oh0 = th * FNN_TILE_H, ow0 = tw * FNN_TILE_W;
    const int ID = (FNN_TILE_D - 1) * p.sd + p.kd;
    const int IH = (FNN_TILE_H - 1) * p.sh + p.kh;
    const int IW = (FNN_TILE_W - 1) * p.sw + p.kw;
    const int IVOX = ID * IH * IW;
    const int T = p.kd * p.kh * p.kw;
    const int cin_total = p.chunks * 16;

    char *sA = smem;
    char *sB = sA + ((IVOX * 32 + 1023) & ~1023);
    int *sOff = (int *)(sB + p.ksteps * NB * 1024);
    float2 *sSS = (float2 *)(sOff + ((IVOX + 3) & ~3));
    int *sTap = (int *)(sSS + cin_total);

    // ---- prologue: halo voxel -> global element offset, tap offsets, scale/shift
    {
        const int id0 = od0 * p.sd - p.pd, ih0 = oh0 * p.sh - p.ph, iw0 = ow0 * p.sw - p.pw;
        for (int v = tid; v < IVOX; v += 256) {
            const int zw = v % IW, zh = (v / IW) % IH, zd = v / (IW * IH);
            const int gd = id0 + zd, gh = ih0 + zh, gw = iw0 + zw;
            const bool ok = gd >= 0 && gd < p.Di && gh >= 0 && gh < p.Hi && gw >= 0 && gw < p.Wi;
            sOff[v] = ok ? ((n * p.Di + gd) * p.Hi + gh) * p.Wi + gw : -1;      // voxel index
        }
        if (tid < 2 * p.ksteps) {
            int off = 0;
            if (tid < T) {
                const int a = tid / (p.kh * p.kw), b = (tid / p.kw) % p.kh, c = tid % p.kw;
                off = ((a * IH + b) * IW + c) * 32;
            }
            sTap[tid] = off;
        }
        for (int c = tid; c < cin_total; c += 256) {
            const int s = (c < p.src[0].C) ? 0 : 1;
            const int cl = c - (s ? p.src[0].C : 0);
            sSS[c] = p.src[s].ss ? make_float2(p.src[s].ss[(size_t)(2 * n) * p.src[s].C + cl], p.src[s].ss[(size_t)(2 * n + 1) * p.src[s].C + cl])
                                 : make_float2(1.f, 0.f);
        }
    }

    // per-lane LDS byte offsets of the 4 column blocks' voxels (k-group folded in)
    int base[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
        const int r = lane & 15;
        const int oh_l = 2 * mb + (r >> 3), ow_l = r & 7;
        base[mb] = ((wave * p.sd * IH + oh_l * p.sh) * IW + ow_l * p.sw) * 32 + ((lane >> 4) & 1) * 16;
    }

    f32x4 acc[4][NB];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};

    __syncthreads();

    const int cg = tid & 1;                 // which 8-channel half of the chunk this thread stages
    for (int ch = 0; ch < p.chunks; ++ch) {
        const int c_glob = ch * 16;
        const int s = (c_glob < p.src[0].C) ? 0 : 1;
        const int c_loc = c_glob - (s ? p.src[0].C : 0) + cg * 8;
        const int sC = p.src[s].C;
        // activation layout (fnn_device.h, SrcDesc): item base + chunk base; sOff holds voxel indices that include the item
        const size_t nvox = (size_t)n * p.Di * p.Hi * p.Wi;
        const int vs = FNN_VS(p.src[s]);
        const f16 *sp = p.src[s].ptr + nvox * sC + (c_loc >> 4) * FNN_CS(p.src[s]) + (c_loc & 15);
        const f16 slope_h = (f16)p.src[s].slope;
        float sc[8], sh[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float2 v = sSS[c_glob + cg * 8 + j];
            sc[j] = v.x; sh[j] = v.y;
        }
        // stage the halo tile of this chunk: global -> normalise + LeakyReLU -> fp16 -> LDS.
        // Loads are issued in batches of 8 before any of them is consumed (one round trip per batch).
        for (int base = tid; base < IVOX * 2; base += 256 * 8) {
            int off[8];
            f16x8 x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int idx = base + u * 256;
                off[u] = idx < IVOX * 2 ? sOff[idx >> 1] : -2;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)       // always a valid address; padding voxels are zeroed below
                x[u] = *(const f16x8 *)(sp + (off[u] >= 0 ? (size_t)off[u] - nvox : 0) * vs);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (off[u] == -2) continue;
                f16x8 o;
                if (off[u] >= 0) {
                    // fp32 fma, one rounding to fp16 (v_fma_mixlo/hi_f16), then LeakyReLU as packed-half
                    // max(y, slope*y) - valid for 0 <= slope <= 1 (slope 1 = identity input)
#pragma unroll
                    for (int j = 0; j < 8; ++j) o[j] = (f16)fmaf((float)x[u][j], sc[j], sh[j]);
                    o = __builtin_elementwise_max(o, o * slope_h);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) o[j] = (f16)0.f;
                }
                *(f16x8 *)(sA + ((base + u * 256) >> 1) * 32 + cg * 16) = o;
            }
        }
        // stage the weight fragments of this chunk (same batching)
        {
            const int per_nb = p.ksteps * 64;                       // uint4 per cout block
            const int total = NB * per_nb;
            for (int base = tid; base < total; base += 256 * 8) {
                uint4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int idx = base + u * 256;
                    const int idc = idx < total ? idx : 0;
                    const int nb = idc / per_nb, r = idc - nb * per_nb;
                    v[u] = ((const uint4 *)(p.wpk + ((size_t)((cb0 + nb) * p.chunks + ch) * p.ksteps) * 512))[r];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int idx = base + u * 256;
                    if (idx < total) ((uint4 *)sB)[idx] = v[u];
                }
            }
        }
        __syncthreads();

        for (int ks = 0; ks < p.ksteps; ++ks) {
            const int toff = sTap[2 * ks + (lane >> 5)];
            f16x8 xf[4];
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) xf[mb] = *(const f16x8 *)(sA + base[mb] + toff);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const f16x8 wf = *(const f16x8 *)(sB + ((nb * p.ksteps + ks) * 64 + lane) * 16);
#pragma unroll
                for (int mb = 0; mb < 4; ++mb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[mb], acc[mb][nb], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // ---- epilogue: bias, fp16 store (4 consecutive channels per lane), statistics
    const int q = lane >> 4, r = lane & 15;
    const int od = od0 + wave;
    float s1[NB][4], s2[NB][4];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int j = 0; j < 4; ++j) { s1[nb][j] = 0.f; s2[nb][j] = 0.f; }

#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
        const int oh = oh0 + 2 * mb + (r >> 3), ow = ow0 + (r & 7);
        const bool ok = od < p.Do && oh < p.Ho && ow < p.Wo;
        const size_t vox = ((size_t)od * p.Ho + oh) * p.Wo + ow;              // inside batch item n
        f16 *outn = p.out + (size_t)n * p.Do * p.Ho * p.Wo * p.Cout;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int co = (cb0 + nb) * 16 + q * 4;
            const float4 bv = *(const float4 *)(p.bias + co);
            f16x4 o;
            o[0] = (f16)(acc[mb][nb][0] + bv.x);
            o[1] = (f16)(acc[mb][nb][1] + bv.y);
            o[2] = (f16)(acc[mb][nb][2] + bv.z);
            o[3] = (f16)(acc[mb][nb][3] + bv.w);
            if (ok) {
                *(f16x4 *)(outn + vox * FNN_OVS(p) + (co >> 4) * FNN_OCS(p) + (co & 15)) = o;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = (float)o[j];
                    s1[nb][j] += v; s2[nb][j] += v * v;
                }
            }
        }
    }
    if (p.stats_out) {
        // reduce over the 16 voxel lanes, then over the 4 waves through LDS
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) {
                    s1[nb][j] += __shfl_xor(s1[nb][j], m, 64);
                    s2[nb][j] += __shfl_xor(s2[nb][j], m, 64);
                }
            }
        float *sRed = (float *)smem;                 // [4 waves][NB*16][2]
        if (r == 0) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = nb * 16 + q * 4 + j;
                    sRed[(wave * NB * 16 + c) * 2] = s1[nb][j];
                    sRed[(wave * NB * 16 + c) * 2 + 1] = s2[nb][j];
                }
        }
        __syncthreads();
        if (tid < NB * 16 * 2) {
            const int c = tid >> 1, which = tid & 1;
            double v = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) v += (double)sRed[(w * NB * 16 + c) * 2 + which];
            double *dst = p.stats_out + (((size_t)n * FNN_STAT_REPL + (blockIdx.x & (FNN_STAT_REPL - 1))) * p.Cout
                                         + cb0 * 16 + c) * 2 + which;
            unsafeAtomicAdd(dst, v);
        }
    }
}

static int lds_pitch(int IW) { return (IW & 7) ? ((IW + 3) & ~7) + 4 : IW; }
// Stride-2 layers keep the plain image (pitch IW): their operand reads (8 voxels 64 bytes apart, two rows) are 2-way
// bank conflicted.  Measured and dropped (round 2): columns stored de-interleaved (even ones first) at a pitch of
// 2 (mod 4) voxels with the channel halves swapped on rows 2, 3, 6, 7, ... - conflict-free reads, bit-identical results,
// but 2-way conflicted ds_write_b128 and 6 % more LDS: 32 -> 64 at 160 x 48 x 48 640 -> 781 us, 64 -> 128 447 -> 514 us.

// ----------------------------------------------------------------------------
// pipelined MFMA conv, weights through LDS per chunk (stride 1)
// ----------------------------------------------------------------------------
// No global load inside the k-loop: vmcnt is an in-order
// counter, so a weight fragment requested after the halo prefetch could not be consumed before the
// whole prefetch had landed, and every chunk stalled on it.  Here the prefetch of chunk c+1 covers the
// halo elements AND the chunk's weight fragments (registers), the k-loop reads both from LDS, and the
// LDS image (single buffered: 2 workgroups per CU even for 8x8x8 tiles) is rewritten between two
// barriers after the MFMAs of chunk c.
template <int NB, int MB, int PF>
__global__ __launch_bounds__(256, 2) void conv3d_lds_kernel(const ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    FNN_STAMP_DECL
    FNN_STAMP();                                             // 0: entry
    constexpr int TD = MB == 2 ? 2 : MB;                   // output tile depth

    // XCD-aware, bijective remap (blocks b and b + 8 share an XCD)
    int t = fnn_xcd_tile(gridDim.x, blockIdx.x);
    const int tw = t % p.tiles_w; t /= p.tiles_w;
    const int th = t % p.tiles_h; t /= p.tiles_h;
    const int td = t % p.tiles_d;
    const int n = t / p.tiles_d;
    const int cb0 = blockIdx.y * NB;

    const int od0 = td * TD, oh0 = th * FNN_TILE_H, ow0 = tw * FNN_TILE_W;
    const int ID = (TD - 1) * p.sd + p.kd, IH = (FNN_TILE_H - 1) * p.sh + p.kh, IW = (FNN_TILE_W - 1) * p.sw + p.kw;
    const int IVOX = ID * IH * IW;
    const int T = p.kd * p.kh * p.kw;
    // LDS image of the halo tile: row pitch PWp voxels, and the two 16-byte channel halves of a voxel are
    // swapped on odd rows (swz) - with PWp = 4 (mod 8) every ds_read_b128 of an MFMA operand is then
    // bank-conflict free (the dense 10-voxel pitch was 2-way conflicted on every read)
    const int swz = p.sw == 1 && (IW & 7) != 0;
    const int PWp = swz ? ((IW + 3) & ~7) + 4 : IW;
    const int abytes = (ID * IH * PWp * 32 + 1023) & ~1023;

    constexpr int WPF = (NB * 14 * 64 + 255) / 256;          // weight uint4 per thread per chunk (<= 14 k-steps)
    char *sA0 = smem;
    char *sW = smem + abytes;                                // [NB][ksteps][64 lanes][16 B] of the current chunk
    int *sTap = (int *)(sW + NB * p.ksteps * 1024);
    float *sBias = (float *)(sTap + 4 * p.ksteps + 4);        // [NB * 16]: read in the epilogue (no global round trip there)

    {
        if (tid < 2 * p.ksteps) {
            int off = 0, par = 0;
            if (tid < T) {
                const int a = tid / (p.kh * p.kw), b = (tid / p.kw) % p.kh, c = tid % p.kw;
                off = ((a * IH + b) * PWp + c) * 32;
                par = swz & b & 1;
            }
            sTap[tid * 2] = off + 16 * par;                  // column for lanes with kgp = 0
            sTap[tid * 2 + 1] = off + 16 * (1 - par);        // kgp = 1
        }
        if (tid >= 64 && tid < 64 + NB * 16) sBias[tid - 64] = p.bias[cb0 * 16 + tid - 64];
    }

    int base[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int r = lane & 15;
        int od_l, oh_l, ow_l;
        mb_coords<MB>(wave, mb, r, od_l, oh_l, ow_l);
        base[mb] = ((od_l * p.sd * IH + oh_l * p.sh) * PWp + ow_l * p.sw) * 32;
    }
    const int kgp = ((lane >> 4) & 1) ^ (swz & ((lane & 15) >> 3));     // channel half after the row swizzle

    f32x4 acc[MB][NB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int per_nb = p.ksteps * 64;                        // 16-byte fragments-lanes per cout block per chunk
    const int wtotal = NB * per_nb;
    f16x8 wr[WPF];                                           // native vector type: stays in registers
    int wofs[WPF];                                           // this thread's weight elements (16-B units), chunk 0
#pragma unroll
    for (int u = 0; u < WPF; ++u) {
        const int idx = tid + u * 256;
        const int idc = idx < wtotal ? idx : wtotal - 1;
        const int nb = (idc >= per_nb) + (idc >= 2 * per_nb) + (idc >= 3 * per_nb);      // NB <= 4: no division
        wofs[u] = (cb0 + nb) * p.chunks * per_nb + idc - nb * per_nb;
    }
    float4 scr[2], shr[2];                                   // 8 scales, 8 shifts of the chunk being prefetched
    float slope_next = 1.f;
    __syncthreads();

    const int cg = tid & 1;
    int offv[PF];                                           // global voxel index of this thread's halo elements
    int ldso[PF];                                           // and where they go in the LDS image
    {
        const int id0 = od0 * p.sd - p.pd, ih0 = oh0 * p.sh - p.ph, iw0 = ow0 * p.sw - p.pw;
        const float rcp_iw = 1.0f / (float)IW, rcp_ih = 1.0f / (float)IH;
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int idx = tid + u * 256;
            const int v = idx >> 1;
            const int row = small_div(v, IW, rcp_iw), zw = v - row * IW;
            const int zd = small_div(row, IH, rcp_ih), zh = row - zd * IH;
            const int gd = id0 + zd, gh = ih0 + zh, gw = iw0 + zw;
            const bool ok = gd >= 0 && gd < p.Di && gh >= 0 && gh < p.Hi && gw >= 0 && gw < p.Wi;
            offv[u] = idx < IVOX * 2 ? (ok ? ((n * p.Di + gd) * p.Hi + gh) * p.Wi + gw : -1) : -2;
            ldso[u] = ((zd * IH + zh) * PWp + zw) * 32 + ((cg ^ (swz & zh & 1)) * 16);
        }
    }
    f16x8 xr[PF];

    auto issue = [&](int ch) {
        const int c_glob = ch * 16;
        const int s = (c_glob < p.src[0].C) ? 0 : 1;
        const int sC = p.src[s].C, c_loc = c_glob - (s ? p.src[0].C : 0) + cg * 8;
        const size_t nvox = (size_t)n * p.Di * p.Hi * p.Wi;     // offv holds voxel indices that include the item
        const int vs = FNN_VS(p.src[s]);                        // activation layout: fnn_device.h, SrcDesc
        const f16 *sp = p.src[s].ptr + nvox * sC + (c_loc >> 4) * FNN_CS(p.src[s]) + (c_loc & 15);
#pragma unroll
        for (int u = 0; u < PF; ++u)                        // unconditional: branches around loads make hipcc drain vmcnt
            xr[u] = *(const f16x8 *)(sp + (offv[u] >= 0 ? (size_t)offv[u] - nvox : 0) * vs);
#pragma unroll
        for (int u = 0; u < WPF; ++u) wr[u] = ((const f16x8 *)p.wpk)[wofs[u] + ch * per_nb];
        slope_next = p.src[s].slope;
        if (p.src[s].ss) {
            const float *q4 = p.src[s].ss + (size_t)(2 * n) * sC + (c_glob - (s ? p.src[0].C : 0)) + cg * 8;
            scr[0] = *(const float4 *)q4; scr[1] = *(const float4 *)(q4 + 4);
            shr[0] = *(const float4 *)(q4 + sC); shr[1] = *(const float4 *)(q4 + sC + 4);
        } else {
            scr[0] = scr[1] = make_float4(1.f, 1.f, 1.f, 1.f);
            shr[0] = shr[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto commit = [&](int ch, char *dst) {
        (void)ch;
        const f16 slope_h = (f16)slope_next;
        const float sc[8] = {scr[0].x, scr[0].y, scr[0].z, scr[0].w, scr[1].x, scr[1].y, scr[1].z, scr[1].w};
        const float sh[8] = {shr[0].x, shr[0].y, shr[0].z, shr[0].w, shr[1].x, shr[1].y, shr[1].z, shr[1].w};
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            if (u * 256 >= IVOX * 2 || offv[u] == -2) continue;
            f16x8 o;
            if (offv[u] >= 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (f16)fmaf((float)xr[u][j], sc[j], sh[j]);
                o = __builtin_elementwise_max(o, o * slope_h);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (f16)0.f;
            }
            *(f16x8 *)(dst + ldso[u]) = o;
        }
#pragma unroll
        for (int u = 0; u < WPF; ++u) {
            const int idx = tid + u * 256;
            if (idx < wtotal) ((f16x8 *)sW)[idx] = wr[u];
        }
    };

    FNN_STAMP();                                             // 1: tables done
    issue(0);
    FNN_STAMP();                                             // 2: first loads issued
    commit(0, sA0);
    __syncthreads();
    FNN_STAMP();                                             // 3: first chunk staged

    auto kloop = [&]() {
        for (int ks = 0; ks < p.ksteps; ++ks) {
            const int toff = sTap[(2 * ks + (lane >> 5)) * 2 + kgp];
            f16x8 xf[MB];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) xf[mb] = *(const f16x8 *)(sA0 + base[mb] + toff);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const f16x8 wf = *(const f16x8 *)(sW + ((nb * p.ksteps + ks) * 64 + lane) * 16);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[mb], acc[mb][nb], 0, 0, 0);
            }
        }
    };
    // All but the last chunk prefetch their successor.  The last chunk is peeled off so that the wait for
    // the prefetch sits on an unconditional path: with `if (more)` around issue/commit, hipcc's waitcnt
    // pass had to assume loads of the previous iteration were still pending and drained vmcnt to 0 in the
    // middle of issue() - the "prefetch" then cost two exposed round trips per chunk.
    for (int ch = 0; ch + 1 < p.chunks; ++ch) {
        issue(ch + 1);                                       // global loads stay in flight during the MFMAs
        kloop();
        FNN_STAMP();                                         // k-loop done
        __syncthreads();                                     // every wave is done reading this chunk
        commit(ch + 1, sA0);
        __syncthreads();
        FNN_STAMP();                                         // next chunk staged
    }
    kloop();
    FNN_STAMP();
    __syncthreads();

    // ---- epilogue: bias, fp16 store, statistics
    {
        float4 bv[NB];                                       // bias of this lane's 4 channels per cout block
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) bv[nb] = *(const float4 *)(sBias + nb * 16 + (lane >> 4) * 4);
        float t1[NB][4], t2[NB][4];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int j = 0; j < 4; ++j) { t1[nb][j] = 0.f; t2[nb][j] = 0.f; }
        tile_epilogue<NB, MB>(p, acc, bv, n, od0, oh0, ow0, cb0, wave, lane, t1, t2);
        if (p.stats_out) stats_to_global<NB>(p, t1, t2, (float *)smem, n, cb0, wave, lane, tid);
    }
    FNN_STAMP();                                             // epilogue done
    FNN_STAMP_FLUSH(p.dbg);
}

static size_t ldsk_lds_bytes(const ConvParams &p, int nb, int mb) {
    const int td = mb == 2 ? 2 : mb;
    const int ID = (td - 1) * p.sd + p.kd, IH = (FNN_TILE_H - 1) * p.sh + p.kh, IW = (FNN_TILE_W - 1) * p.sw + p.kw;
    const int pitch = p.sw == 1 ? lds_pitch(IW) : IW;
    size_t b = (size_t)((ID * IH * pitch * 32 + 1023) & ~1023) + (size_t)nb * p.ksteps * 1024;
    b += 4 * p.ksteps * 4 + 16 + (size_t)nb * 16 * 4 + 64;
    const size_t red = (size_t)4 * nb * 16 * 2 * 4;
    return b > red ? b : red;
}

template <int NB, int MB, int PF = 8>
static int launch_ldsk(ConvParams p, hipStream_t st) {
    constexpr int TD = MB == 2 ? 2 : MB;
    p.tile_d = TD;
    p.tiles_d = (p.Do + TD - 1) / TD;
    p.tiles_h = (p.Ho + FNN_TILE_H - 1) / FNN_TILE_H;
    p.tiles_w = (p.Wo + FNN_TILE_W - 1) / FNN_TILE_W;
    const size_t lds = ldsk_lds_bytes(p, NB, MB);
    dim3 grid(p.N * p.tiles_d * p.tiles_h * p.tiles_w, (p.Cout / 16) / NB);
    return fnn_launch_lds<conv3d_lds_kernel<NB, MB, PF>>(grid, dim3(256), lds, st, p);
}

// ----------------------------------------------------------------------------
// persistent MFMA conv (stride 1) for layers with many tiles
// ----------------------------------------------------------------------------
// The thin full-resolution layers do only a few hundred MFMA cycles per tile, so
// a one-tile-per-workgroup kernel is bound by its own latency chain (table
// set-up, one global round trip for the halo, weight fetch, epilogue).  Here a
// workgroup owns a contiguous range of tiles and pipelines ACROSS tiles:
//   * all weight fragments of its cout group are loaded into LDS once;
//   * work item = (tile, 16-channel chunk); the halo loads (and the scale/shift
//     of the producer's InstanceNorm) of item i+1 are in flight while item i
//     runs on the matrix cores; one barrier per item;
//   * InstanceNorm statistics are kept in registers across the tiles of one
//     batch item and flushed with one set of atomics per workgroup.
template <int NB, int MB, bool WRES, int KS, int CH, int PF = 8, bool SBUF = false>
__global__ __launch_bounds__(256, (NB == 1 && MB == 4 && WRES && PF == 4) ? 3 : 2) void conv3d_persist_kernel(const ConvParams p, const int total_tiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    FNN_STAMP_DECL
    constexpr int TD = MB;                                            // MB = 2: the strided 2 x 8 x 8 tile (mb_coords<2>)

    const int ID = (TD - 1) * p.sd + p.kd, IH = (FNN_TILE_H - 1) * p.sh + p.kh, IW = (FNN_TILE_W - 1) * p.sw + p.kw;
    const int IVOX = ID * IH * IW;
    const int T = p.kd * p.kh * p.kw;
    const int TS = p.chunks * p.ksteps;
    const int swz = p.sw == 1 && (IW & 7) != 0;                       // LDS image: see conv3d_lds_kernel
    const int PWp = swz ? ((IW + 3) & ~7) + 4 : IW;
    const int abytes = (ID * IH * PWp * 32 + 1023) & ~1023;
    const int cb0 = blockIdx.y * NB;

    // WRES: all weight fragments of the cout group stay in LDS, halo tile double buffered (one barrier per
    // item).  !WRES: the weights of one chunk travel with the halo prefetch, single buffers, two barriers.
    // SBUF (with WRES): resident weights next to a SINGLE halo buffer - for tiles whose double buffer would not leave
    // room for two workgroups per CU (the strided full-resolution conv: 37 KB of halo, 28 KB of weights).
    constexpr int NBUF = (WRES && !SBUF) ? 2 : 1;
    constexpr int WPF = WRES ? 1 : (NB * 14 * 64 + 255) / 256;
    char *sA0 = smem;
    char *sW = smem + NBUF * abytes;                                 // [NB][TS or ksteps][64 lanes][16 B]
    int *sTap = (int *)(sW + NB * (WRES ? TS : p.ksteps) * 1024);
    double *sRed = (double *)(sTap + 64);                             // [4 waves][NB*16][2]

    // contiguous tile range of this workgroup; consecutive ranges share an XCD
    int t_begin, t_end;
    {
        const int nwg = gridDim.x, bid = blockIdx.x;
        const int g = fnn_xcd_tile(nwg, bid);
        t_begin = (int)((long long)total_tiles * g / nwg);
        t_end = (int)((long long)total_tiles * (g + 1) / nwg);
    }
    if (t_begin >= t_end) return;

    // ---- one-time set-up: weights -> LDS (WRES), tap offsets, this thread's halo coordinates
    if (WRES) {
        for (int idx = tid; idx < NB * TS * 64; idx += 256) {
            const int nb = idx / (TS * 64), r = idx - nb * (TS * 64);
            ((uint4 *)sW)[idx] = ((const uint4 *)(p.wpk + (size_t)(cb0 + nb) * TS * 512))[r];
        }
    }
    const int per_nb = p.ksteps * 64, wtotal = NB * per_nb;
    f16x8 wr[WPF];
    int wofs[WPF];
#pragma unroll
    for (int u = 0; u < WPF; ++u) {
        const int idx = tid + u * 256;
        const int idc = idx < wtotal ? idx : wtotal - 1;
        const int nb = idc / per_nb, r = idc - nb * per_nb;
        wofs[u] = (cb0 + nb) * p.chunks * per_nb + r;
    }
    if (tid < 2 * p.ksteps) {
        int off = 0, par = 0;
        if (tid < T) {
            const int a = tid / (p.kh * p.kw), b = (tid / p.kw) % p.kh, c = tid % p.kw;
            off = ((a * IH + b) * PWp + c) * 32;
            par = swz & b & 1;
        }
        sTap[tid * 2] = off + 16 * par;
        sTap[tid * 2 + 1] = off + 16 * (1 - par);
    }
    const int cg = tid & 1;
    // packed halo coords of this thread's elements: registers, or - for the 12-element prefetch of the strided kernels,
    // which otherwise spill - a table in LDS behind the statistics scratch
    // (tried for the strided kernels' 12-element prefetch, which spills 20-48 B per lane: the table's 12 KB push the
    // 32 -> 64 strided conv over 80 KB, one workgroup per CU: -6 % end to end; the spill stays)
    constexpr bool REL_LDS = false && PF >= 12;
    int *sRel = (int *)(sRed + 4 * NB * 16 * 2) + tid;
    int relr[REL_LDS ? 1 : PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const int idx = tid + u * 256;
        const int v = idx >> 1;
        const int zw = v % IW, zh = (v / IW) % IH, zd = v / (IW * IH);
        const int rv = idx < IVOX * 2 ? (zd << 16) | (zh << 8) | zw : -1;
        if (REL_LDS) sRel[u * 256] = rv; else relr[REL_LDS ? 0 : u] = rv;
    }
#define FNN_REL(u) (REL_LDS ? sRel[(u) * 256] : relr[REL_LDS ? 0 : (u)])
    int base[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int r = lane & 15;
        int od_l, oh_l, ow_l;
        mb_coords<MB>(wave, mb, r, od_l, oh_l, ow_l);
        base[mb] = ((od_l * p.sd * IH + oh_l * p.sh) * PWp + ow_l * p.sw) * 32;
    }
    const int kgp = ((lane >> 4) & 1) ^ (swz & ((lane & 15) >> 3));

    f32x4 acc[MB][NB];
    // statistics: fp32 only WITHIN one tile (same grouping as the one-tile-per-workgroup kernels), double
    // across tiles - sums of fp16-valued numbers in double are exact, so the result does not depend on how
    // tiles are distributed over workgroups.  The double accumulators live in LDS (one slot per wave).
    for (int i = tid; i < 4 * NB * 16 * 2; i += 256) sRed[i] = 0.0;
    // per-lane running sums between flushes (double): a tile adds its fp32 lane partials, the 16 lanes of a row meet
    // only when the statistics are flushed - instead of four DPP steps per value and an LDS read-add-write per tile
    double dsum[NB][4][2];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int j = 0; j < 4; ++j) { dsum[nb][j][0] = 0.0; dsum[nb][j][1] = 0.0; }

    float4 bv[NB];                                                    // bias of this lane's 4 channels per cout block
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) bv[nb] = *(const float4 *)(p.bias + (cb0 + nb) * 16 + (lane >> 4) * 4);

    int offv[PF];
    f16x8 xr[PF];
    float4 scr[2], shr[2];                                            // 8 scales, 8 shifts of the next item
    float slope_next = 1.f;

    auto tile_coords = [&](int t, int &n, int &od0, int &oh0, int &ow0) {
        const int tw = t % p.tiles_w; t /= p.tiles_w;
        const int th = t % p.tiles_h; t /= p.tiles_h;
        const int td = t % p.tiles_d;
        n = t / p.tiles_d;
        od0 = td * TD; oh0 = th * FNN_TILE_H; ow0 = tw * FNN_TILE_W;
    };
    // consecutive tiles: step the coordinates instead of dividing again (w fastest, then h, d, batch item)
    auto next_tile = [&](int &n, int &od0, int &oh0, int &ow0) {
        ow0 += FNN_TILE_W;
        if (ow0 >= p.tiles_w * FNN_TILE_W) {
            ow0 = 0; oh0 += FNN_TILE_H;
            if (oh0 >= p.tiles_h * FNN_TILE_H) {
                oh0 = 0; od0 += TD;
                if (od0 >= p.tiles_d * TD) { od0 = 0; ++n; }
            }
        }
    };
    // offv = voxel index inside batch item n (or -1 for conv padding); the item's base pointer is uniform
    auto set_offsets = [&](int od0, int oh0, int ow0) {
        const int id0 = od0 * p.sd - p.pd, ih0 = oh0 * p.sh - p.ph, iw0 = ow0 * p.sw - p.pw;
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int rel_u = FNN_REL(u);
            const unsigned gd = (unsigned)(id0 + (rel_u >> 16)), gh = (unsigned)(ih0 + ((rel_u >> 8) & 255)),
                           gw = (unsigned)(iw0 + (rel_u & 255));
            const bool ok = rel_u >= 0 && gd < (unsigned)p.Di && gh < (unsigned)p.Hi && gw < (unsigned)p.Wi;
            // two 24-bit mads (full rate; v_mul_lo_u32 is quarter rate) instead of a held offset: Di * Hi < 2^24 (launcher)
            offv[u] = ok ? (int)(__umul24(__umul24(gd, (unsigned)p.Hi) + gh, (unsigned)p.Wi) + gw) : -1;
        }
    };
    auto issue = [&](int n, int ch) {
        const int c_glob = ch * 16;
        const int s = (c_glob < p.src[0].C) ? 0 : 1;
        const int c_loc = c_glob - (s ? p.src[0].C : 0) + cg * 8;
        const int sC = p.src[s].C;
        const int vs = FNN_VS(p.src[s]);                    // activation layout: fnn_device.h, SrcDesc
        const char *sp = (const char *)(p.src[s].ptr + (size_t)n * p.Di * p.Hi * p.Wi * sC + (c_loc >> 4) * FNN_CS(p.src[s]) + (c_loc & 15));   // uniform base
        slope_next = p.src[s].slope;
        // scale / shift first (vmcnt retires in order: commit() needs them before the first halo element) and
        // unconditionally: the identity table stands in for a source without InstanceNorm
        const float *qs = p.src[s].ss ? p.src[s].ss + (size_t)(2 * n) * sC + c_loc : p.ident_ss + c_loc;   // (fnn_ss_rows: one more spilled SGPR here)
        const float *qh = p.src[s].ss ? qs + sC : p.ident_ss + 512 + c_loc;
        scr[0] = *(const float4 *)qs; scr[1] = *(const float4 *)(qs + 4);
        shr[0] = *(const float4 *)qh; shr[1] = *(const float4 *)(qh + 4);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < PF; ++u)                        // unconditional: branches around loads make hipcc drain vmcnt
            xr[u] = *(const f16x8 *)(sp + (unsigned)((offv[u] >= 0 ? offv[u] : 0) * vs * 2));
        if (!WRES) {
#pragma unroll
            for (int u = 0; u < WPF; ++u) wr[u] = ((const f16x8 *)p.wpk)[wofs[u] + ch * per_nb];
        }
    };
    auto commit = [&](char *dst) {
        const f16 slope_h = (f16)slope_next;
        const float sc[8] = {scr[0].x, scr[0].y, scr[0].z, scr[0].w, scr[1].x, scr[1].y, scr[1].z, scr[1].w};
        const float sh[8] = {shr[0].x, shr[0].y, shr[0].z, shr[0].w, shr[1].x, shr[1].y, shr[1].z, shr[1].w};
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            if (u * 256 >= IVOX * 2) continue;                          // uniform: no thread has an element u
            // branch-free: with `if (offv >= 0)` around the arithmetic the waits for the prefetch sat in conditional
            // blocks, and hipcc then had to assume at the loop head that loads (and the stores behind them) were
            // still pending - it drained the previous tile's stores before every prefetch
            f16x8 o = fnn_norm_leaky8(xr[u], sc, sh, slope_h);
            if (offv[u] < 0) o = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};             // the conv's zero padding
            const int rel_u = FNN_REL(u);
            const int zd = rel_u >> 16, zh = (rel_u >> 8) & 255, zw = rel_u & 255;
            if (rel_u >= 0) *(f16x8 *)(dst + ((zd * IH + zh) * PWp + zw) * 32 + ((cg ^ (swz & zh & 1)) * 16)) = o;
        }
        if (!WRES) {
#pragma unroll
            for (int u = 0; u < WPF; ++u) {
                const int idx = tid + u * 256;
                if (idx < wtotal) ((f16x8 *)sW)[idx] = wr[u];
            }
        }
    };
    auto flush_stats = [&](int n) {
        if (!p.stats_out) return;
        {
            const int q = lane >> 4;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double a = row16_sum_f64(dsum[nb][j][0]), b = row16_sum_f64(dsum[nb][j][1]);
                    if ((lane & 15) == 0) {                           // one lane per (wave, channel)
                        double *slot = sRed + (wave * NB * 16 + nb * 16 + q * 4 + j) * 2;
                        slot[0] = a; slot[1] = b;
                    }
                    dsum[nb][j][0] = 0.0; dsum[nb][j][1] = 0.0;
                }
        }
        __syncthreads();
        if (tid < NB * 16 * 2) {
            const int c = tid >> 1, which = tid & 1;
            double v = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) { v += sRed[(w * NB * 16 + c) * 2 + which]; sRed[(w * NB * 16 + c) * 2 + which] = 0.0; }
            unsafeAtomicAdd(p.stats_out + (((size_t)n * FNN_STAT_REPL + (blockIdx.x & (FNN_STAT_REPL - 1))) * p.Cout
                                           + cb0 * 16 + c) * 2 + which, v);
        }
        __syncthreads();
    };

    int n_cur, od0, oh0, ow0;
    tile_coords(t_begin, n_cur, od0, oh0, ow0);
    set_offsets(od0, oh0, ow0);
    issue(n_cur, 0);
    commit(sA0);
    __syncthreads();
    int toffs[14];                                                    // this lane's tap offset per k-step (KS known);
    if (KS) {                                                         // read after the barrier that publishes sTap
#pragma unroll
        for (int ks = 0; ks < (KS < 14 ? KS : 14); ++ks) toffs[ks] = sTap[(2 * ks + (lane >> 5)) * 2 + kgp];
    }

    int buf = 0;
    for (int t = t_begin; t < t_end; ++t) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
        int n_next = n_cur, nod0 = od0, noh0 = oh0, now0 = ow0;
        constexpr int CHU = CH ? CH : 1;
#pragma unroll CHU
        for (int ch = 0; ch < (CH ? CH : p.chunks); ++ch) {
            // prefetch the next work item.  The very last item prefetches itself again (a few redundant, cached
            // loads) so that issue / commit sit on an unconditional path: hipcc's waitcnt pass is then exact
#ifdef FNN_STAMPS
            const bool stamp_it = t == t_begin + 2 && ch == 0;
            if (stamp_it) FNN_STAMP();                           // 0: item start
#endif
            const bool last_chunk = ch + 1 == (CH ? CH : p.chunks);
            if (last_chunk) {
                if (t + 1 < t_end) next_tile(n_next, nod0, noh0, now0);
                set_offsets(nod0, noh0, now0);
                issue(n_next, 0);
            } else {
                issue(n_cur, ch + 1);
            }
#ifdef FNN_STAMPS
            if (stamp_it) FNN_STAMP();                           // 1: prefetch issued
#endif
            const char *sA = sA0 + (NBUF == 2 ? buf * abytes : 0);
#pragma unroll
            for (int ks = 0; ks < (KS ? KS : p.ksteps); ++ks) {
                const int toff = KS ? toffs[ks < 14 ? ks : 0] : sTap[(2 * ks + (lane >> 5)) * 2 + kgp];
                f16x8 xf[MB];
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) xf[mb] = *(const f16x8 *)(sA + base[mb] + toff);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const f16x8 wf = *(const f16x8 *)(sW + ((size_t)(WRES ? nb * TS + ch * p.ksteps + ks : nb * p.ksteps + ks) * 64 + lane) * 16);
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[mb], acc[mb][nb], 0, 0, 0);
                }
            }
#ifdef FNN_STAMPS
            if (stamp_it) FNN_STAMP();                           // 2: k-loop done
#endif
            if (last_chunk) {
                // epilogue of this tile: bias, fp16 store, statistics (fp32 within the tile, double across tiles)
                float t1[NB][4], t2[NB][4];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int j = 0; j < 4; ++j) { t1[nb][j] = 0.f; t2[nb][j] = 0.f; }
                tile_epilogue<NB, MB>(p, acc, bv, n_cur, od0, oh0, ow0, cb0, wave, lane, t1, t2);
                if (p.stats_out) {
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            dsum[nb][j][0] += (double)t1[nb][j];
                            dsum[nb][j][1] += (double)t2[nb][j];
                        }
                }
                // commit() is duplicated on purpose: on this path hipcc can wait for the (older) prefetch loads
                // alone - vmcnt(number of epilogue stores) - instead of vmcnt(0) after a merge point, which would
                // expose the store acknowledgement latency once per tile
                if (NBUF == 1) __syncthreads();                  // single buffers: everybody is done reading
                commit(sA0 + (NBUF == 2 ? (buf ^ 1) * abytes : 0));
            } else {
                if (NBUF == 1) __syncthreads();
                commit(sA0 + (NBUF == 2 ? (buf ^ 1) * abytes : 0));
            }
#ifdef FNN_STAMPS
            if (stamp_it) FNN_STAMP();                           // 3: epilogue + commit done
#endif
            __syncthreads();
#ifdef FNN_STAMPS
            if (stamp_it) FNN_STAMP();                           // 4: commit + barrier done
#endif
            buf ^= 1;
        }
        if (n_next != n_cur || t + 1 == t_end) flush_stats(n_cur);
        n_cur = n_next; od0 = nod0; oh0 = noh0; ow0 = now0;
    }
    FNN_STAMP_FLUSH(p.dbg);
#undef FNN_REL
}

static size_t persist_lds_bytes(const ConvParams &p, int nb, int mb, bool wres, bool sbuf = false, int pf = 8) {
    const int ID = (mb - 1) * p.sd + p.kd, IH = (FNN_TILE_H - 1) * p.sh + p.kh, IW = (FNN_TILE_W - 1) * p.sw + p.kw;
    const size_t ab = (size_t)((ID * IH * (p.sw == 1 ? lds_pitch(IW) : IW) * 32 + 1023) & ~1023);
    return (wres && !sbuf ? 2 : 1) * ab + (size_t)nb * (wres ? p.chunks : 1) * p.ksteps * 1024 + 256 + (size_t)4 * nb * 16 * 2 * 8 +
           (false && pf >= 12 ? (size_t)pf * 256 * 4 : 0);
}

template <int NB, int MB, bool WRES, int KS, int CH = 0, int PF = 8, bool SBUF = false>
static int launch_persist_ks(ConvParams p, int wgs_per_cu, hipStream_t st, int gx_exact = 0) {
    p.tile_d = MB;
    p.tiles_d = (p.Do + MB - 1) / MB;
    p.tiles_h = (p.Ho + FNN_TILE_H - 1) / FNN_TILE_H;
    p.tiles_w = (p.Wo + FNN_TILE_W - 1) / FNN_TILE_W;
    const int total = p.N * p.tiles_d * p.tiles_h * p.tiles_w;
    p.ident_ss = conv3d_identity_ss();
    if (!p.ident_ss) return -2;
    const size_t lds = persist_lds_bytes(p, NB, MB, WRES, SBUF, PF);
    int gx = gx_exact > 0 ? gx_exact : 256 * wgs_per_cu;
    if (gx > total) gx = total;
    dim3 grid(gx, (p.Cout / 16) / NB);
    return fnn_launch_lds<conv3d_persist_kernel<NB, MB, WRES, KS, CH, PF, SBUF>>(grid, dim3(256), lds, st, p, total);
}

// the instantiations conv_choose_linear can choose: (NB, MB, WRES, KS, CH, PF, SBUF) = c.t
static int launch_persist(const ConvParams &p, const ConvChoice &c, hipStream_t st) {
    const int mb = c.t[1], wres = c.t[2], ks = c.t[3], ch = c.t[4];
    if (c.t[0] == 2) return launch_persist_ks<2, 2, true, 0, 1, 12, true>(p, c.wpc, st, c.gx);
    if (ch == 1) return launch_persist_ks<1, 4, true, 5, 1, 4>(p, c.wpc, st);
    if (ch == 2) return launch_persist_ks<1, 4, true, 5, 2, 4>(p, c.wpc, st);
    if (mb == 8) {
        if (wres) return ks == 5 ? launch_persist_ks<1, 8, true, 5>(p, c.wpc, st) : launch_persist_ks<1, 8, true, 0>(p, c.wpc, st);
        return ks == 5 ? launch_persist_ks<1, 8, false, 5>(p, c.wpc, st) : launch_persist_ks<1, 8, false, 14>(p, c.wpc, st);
    }
    if (wres) return ks == 5 ? launch_persist_ks<1, 4, true, 5>(p, c.wpc, st) : launch_persist_ks<1, 4, true, 0>(p, c.wpc, st);
    return launch_persist_ks<1, 4, false, 5>(p, c.wpc, st);
}

size_t conv3d_lds_bytes(const ConvParams &p, int nb) {
    const int ID = (FNN_TILE_D - 1) * p.sd + p.kd;
    const int IH = (FNN_TILE_H - 1) * p.sh + p.kh;
    const int IW = (FNN_TILE_W - 1) * p.sw + p.kw;
    const int IVOX = ID * IH * IW;
    size_t b = (size_t)((IVOX * 32 + 1023) & ~1023);
    b += (size_t)p.ksteps * nb * 1024;
    b += (size_t)((IVOX + 3) & ~3) * 4;
    b += (size_t)p.chunks * 16 * 8;
    b += 2 * p.ksteps * 4 + 64;
    const size_t red = (size_t)4 * nb * 16 * 2 * 4;
    return b > red ? b : red;
}

// [0, 512): ones, [512, 1024): zeros - the "no InstanceNorm on this source" scale / shift rows, so that kernels
// can load scale / shift unconditionally (a branch around those loads makes the waitcnt bookkeeping of the
// persistent kernel conservative: it then waited for the previous tile's store acknowledgements before every prefetch)
const float *conv3d_identity_ss() {
    static const float *tab[16] = {nullptr};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    if (!tab[dev]) {
        float h[1024];
        for (int i = 0; i < 512; ++i) { h[i] = 1.f; h[512 + i] = 0.f; }
        float *d = nullptr;                                       // made once per process and device, never freed: no owner (owned.h)
        if (hipMalloc((void **)&d, sizeof(h)) != hipSuccess) return nullptr;
        if (hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
        tab[dev] = d;
    }
    return tab[dev];
}

// SrcDesc::ssh rows of a source without InstanceNorm: per group of 8 channels 8 x 1.0 then 8 x 0.0 (fp16), 512 channels
const unsigned short *conv3d_identity_ssh() {
    static const unsigned short *tab[16] = {nullptr};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    if (!tab[dev]) {
        unsigned short h[1024];
        for (int i = 0; i < 1024; ++i) h[i] = (i & 8) ? 0 : 0x3c00;
        unsigned short *d = nullptr;                              // (never freed either)
        if (hipMalloc((void **)&d, sizeof(h)) != hipSuccess) return nullptr;
        if (hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
        tab[dev] = d;
    }
    return tab[dev];
}

int conv3d_pick_nb(int nblk) { return (nblk % 4 == 0) ? 4 : (nblk % 2 == 0) ? 2 : 1; }

template <int NB>
static int launch_conv_nb(ConvParams p, hipStream_t st) {
    p.tile_d = FNN_TILE_D;
    p.tiles_d = (p.Do + FNN_TILE_D - 1) / FNN_TILE_D;
    p.tiles_h = (p.Ho + FNN_TILE_H - 1) / FNN_TILE_H;
    p.tiles_w = (p.Wo + FNN_TILE_W - 1) / FNN_TILE_W;
    const size_t lds = conv3d_lds_bytes(p, NB);
    dim3 grid(p.N * p.tiles_d * p.tiles_h * p.tiles_w, (p.Cout / 16) / NB);
    return fnn_launch_lds<conv3d_mfma_kernel<NB>>(grid, dim3(256), lds, st, p);
}

static void set_persist(ConvChoice &c, int nb, int mb, int wres, int ks, int ch, int pf, int sbuf, int wpc) {
    c.kernel = CK_PERSIST;
    const int t[7] = {nb, mb, wres, ks, ch, pf, sbuf};
    for (int i = 0; i < 7; ++i) c.t[i] = t[i];
    c.wpc = wpc;
    snprintf(c.name, sizeof c.name, "conv3d_persist_kernel<%d,%d,%d,%d,%d,%d,%d>", nb, mb, wres, ks, ch, pf, sbuf);
}

static void set_ldsk(ConvChoice &c, int nb, int mb, int pf) {
    c.kernel = CK_LDSK; c.t[0] = nb; c.t[1] = mb; c.t[2] = pf;
    snprintf(c.name, sizeof c.name, "conv3d_lds_kernel<%d,%d,%d>", nb, mb, pf);
}

// The linear-tap kernels (FNN_PACK_LINEAR): persistent and one-tile-per-workgroup forms for stride 1, the strided kernels,
// and the generic kernel that takes every shape.
static bool conv_choose_linear(const ConvParams &p_in, const ConvOverrides &o, ConvChoice &c) {
    ConvParams p = p_in;
    c.packing = FNN_PACK_LINEAR; c.ksteps = conv3d_ksteps(FNN_PACK_LINEAR, p.kd * p.kh * p.kw); c.chunks = p.chunks;
    p.ksteps = c.ksteps;
    p.tiles_h = (p.Ho + FNN_TILE_H - 1) / FNN_TILE_H;
    p.tiles_w = (p.Wo + FNN_TILE_W - 1) / FNN_TILE_W;
    // decisions use the engine's planned batch, not this call's, so that a layer always runs the same
    // variant (bit-reproducible statistics whatever the number of patches in the batch)
    const int plan_n = p.plan_N > 0 ? p.plan_N : p.N;
    int nb = conv3d_pick_nb(p.Cout / 16);
    if (!o.conv_v1 && p.sd == 1 && p.sh == 1 && p.sw == 1) {
        // (cout blocks per workgroup, column blocks per wave): prefer the most work per staged byte,
        // but small feature maps need workgroups first - the deep layers are latency bound otherwise
        const int nblk = p.Cout / 16;
        // ((4, 4) - four cout blocks per workgroup - kept 44 B of scratch per lane and is gone: round 3)
        const int cand[4][2] = {{2, 8}, {2, 4}, {1, 8}, {1, 4}};
        int pick = -1, best = -1;
        long long best_wgs = -1;
        for (int i = 0; i < 4; ++i) {
            const int cnb = cand[i][0], cmb = cand[i][1];
            if (nblk % cnb) continue;
            if (cmb == 8 && p.Do < 8) continue;
            const long long wgs = (long long)plan_n * ((p.Do + cmb - 1) / cmb) * p.tiles_h * p.tiles_w * (nblk / cnb);
            if (pick < 0 && wgs >= 768) pick = i;
            if (wgs > best_wgs) { best_wgs = wgs; best = i; }
        }
        if (pick < 0) pick = best;
        nb = cand[pick][0];
        const int mbsel = cand[pick][1];
        // one cout block only: the NB = 2 / 4 forms need 272-644 B of scratch per lane next to their accumulators
        if (p.ksteps <= 14 && nb == 1) {
            // persistent variants: a workgroup walks a range of tiles and prefetches across tile boundaries.
            // Weights resident in LDS when the whole cout group fits next to a double-buffered halo tile with
            // 2 workgroups per CU, otherwise they travel with the prefetch chunk by chunk.
            for (int mb = mbsel; mb >= 4; mb -= 4) {
                const long long tiles = (long long)plan_n * ((p.Do + mb - 1) / mb) * p.tiles_h * p.tiles_w;
                if (tiles < 256LL * 2 * 4) continue;
                for (int wres = 1; wres >= 0; --wres) {
                    // travelling weights only for the unrolled forms (9 taps; 27 taps at 8 planes): a 1x1x1 (or 3-tap) layer whose
                    // weights do not fit - more than 800 input channels - takes the one-tile-per-workgroup kernels below (round 3:
                    // instantiations that no shape short of that reached)
                    if (!wres && !(p.ksteps == 5 || (p.ksteps == 14 && mb == 8))) continue;
                    const size_t lds = persist_lds_bytes(p, nb, mb, wres != 0);
                    const int per_cu = (int)((160 * 1024) / lds);
                    if (per_cu < 2) continue;
                    const int wpc = per_cu > 3 ? 3 : per_cu;
                    if (wres && mb == 8 && p.ksteps == 5 && (p.chunks == 1 || p.chunks == 2)) {
                        // 4-deep tiles with a 4-element prefetch need 138-151 VGPRs and 36 KB of LDS: three workgroups per CU instead
                        // of two - more bytes in flight for these HBM-bound layers (+0.8 % on the benchmark).  Four (round 2: scale / shift
                        // through scalar loads, forced to 128 VGPRs: 44-132 B of scratch): 740 -> 895 us per launch; the scalar loads alone,
                        // at three workgroups: 817 us - SMEM shares lgkmcnt with the LDS reads of the k-loop and returns out of order, so every
                        // wait becomes a full drain
                        // (the 8-deep forms of these two were reachable through an A-B knob only and are gone: round 3)
                        const int ivox4 = (3 * p.sd + p.kd) * ((FNN_TILE_H - 1) * p.sh + p.kh) * ((FNN_TILE_W - 1) * p.sw + p.kw);
                        if (ivox4 * 2 <= 4 * 256 && persist_lds_bytes(p, 1, 4, true) * 3 <= 160 * 1024) {
                            set_persist(c, 1, 4, 1, 5, p.chunks, 4, 0, 3);
                            return true;
                        }
                    }
                    // fully unrolled k-loops for the two common tap counts (9 taps = 5 k-steps, 27 taps = 14); 27 linear taps (a
                    // 3 x 3 x 3 layer the depth-shift kernels refuse: >= 2^23 voxels per item): 8-deep tiles never fit with resident
                    // weights, so that is the one unrolled form; whatever else turns up runs the runtime k-loop
                    set_persist(c, 1, mb, wres, p.ksteps == 5 ? 5 : wres ? 0 : 14, 0, 8, 0, wpc);
                    return true;
                }
            }
        }
        if (p.ksteps <= 14) {
            set_ldsk(c, nb, mbsel, 8);
            return true;
        }
    }
    if (!o.conv_v1 && s2_choose(p, c)) return true;          // stride (2, 2, 2) with whole groups of 64 output channels (conv3d_s2.hip)
    if (!o.conv_v1 && p.ksteps <= 14) {
        // strided convs: 2 x 8 x 8 output tile, up to 16 halo elements per thread, <= 2 cout blocks
        const int nbs = (p.Cout / 16) % 2 == 0 ? 2 : 1;
        const int ID = (2 - 1) * p.sd + p.kd, IH = (FNN_TILE_H - 1) * p.sh + p.kh, IW = (FNN_TILE_W - 1) * p.sw + p.kw;
        // persistent form (tile ranges, cross-tile prefetch) when every workgroup gets a good number of tiles:
        // with one tile per workgroup and a single 16-channel chunk nothing hides the halo round trip
        const long long tiles = (long long)plan_n * ((p.Do + 1) / 2) * p.tiles_h * p.tiles_w;
        const int groups = (p.Cout / 16) / nbs;
        // weights resident next to a single halo buffer: the 28 KB of weight fragments no longer travel with every 37 KB halo
        // tile (+1 % on the benchmark).  (The forms whose weights travel with every halo tile - one chunk without room for
        // resident weights, or several chunks - kept 20 / 48 B of scratch per lane and are gone: those layers take the
        // one-tile-per-workgroup strided kernels below.  Round 3: no kernel of the library keeps scratch.)
        if (nbs == 2 && ID * IH * IW * 2 <= 12 * 256 && persist_lds_bytes(p, 2, 2, false, false, 12) <= 80 * 1024 &&
            tiles >= 8LL * (512 / groups) && 512 / groups >= 8 && p.chunks == 1 && persist_lds_bytes(p, 2, 2, true, true, 12) <= 80 * 1024) {
            set_persist(c, 2, 2, 1, 0, 1, 12, 1, 2);
            c.gx = 512 / groups;                               // 2 resident workgroups per CU over all cout groups
            return true;
        }
        if (ID * IH * IW * 2 <= 16 * 256 && ldsk_lds_bytes(p, nbs, 2) <= 80 * 1024) {
            set_ldsk(c, nbs, 2, ID * IH * IW * 2 <= 8 * 256 ? 8 : 16);
            return true;
        }
    }
    if (nb == 4 && conv3d_lds_bytes(p, 4) > 160 * 1024) nb = 2;
    if (conv3d_lds_bytes(p, nb) > 160 * 1024) return false;
    c.kernel = CK_NB; c.t[0] = nb;
    snprintf(c.name, sizeof c.name, "conv3d_mfma_kernel<%d> (generic fallback)", nb);
    return true;
}

ConvOverrides ConvOverrides::from_env() {
    ConvOverrides o;
    o.conv_v1 = fnn_knob("FNN_CONV_V1") != nullptr;           // the test of the generic kernel
    o.no_row = fnn_knob("FNN_NO_ROW") != nullptr;
    o.no_stem_row = fnn_knob("FNN_NO_STEM_ROW") != nullptr;
    o.no_zr6 = fnn_knob("FNN_NO_ZR6") != nullptr;
    o.no_zrp = fnn_knob("FNN_NO_ZRP") != nullptr;             // conv3d_zr_kernel on the padded order (the tests compare the two orders' bits)
    o.no_zq12 = fnn_knob("FNN_NO_ZQ12") != nullptr;           // conv3d_zr12_kernel instead (the tests compare the two kernels' bits)
    o.no_zsw = fnn_knob("FNN_NO_ZSW") != nullptr;
    o.no_zp = fnn_knob("FNN_NO_ZP") != nullptr;
    o.zp_no_half = fnn_knob("FNN_ZP_NO_HALF") != nullptr;
    o.zps_no_half = fnn_knob("FNN_ZPS_NO_HALF") != nullptr;
    if (const char *v = fnn_knob("FNN_ZR_MIN_WGS")) o.zr_min_wgs = atoi(v);   // tools/fp8_sensitivity.py
    if (const char *v = fnn_knob("FNN_FP8_LEVELS")) o.fp8_levels = atoi(v);   // tools/fp8_sensitivity.py
    return o;
}

// The order of the families.  A fused layer: the row kernels, else the tile form.  Otherwise the plane kernels (ZP), the
// depth-shift kernels (ZS / ZR), the row kernels, then the linear-tap kernels.
bool conv_choose(const ThinParams &tp, const ConvOverrides &o, ConvChoice &c) {
    c = ConvChoice{};
    if (tp.fuse) {
        ConvChoice t;
        if (!thin_choose(tp, t)) return false;
        if (!row_choose(tp, o, c)) c = t;
        return true;
    }
    const ConvParams &p = tp.c;
    // the kernels address one batch item with 32-bit byte offsets (buffer stores, SGPR base + VGPR offset loads)
    const unsigned long long out_item = 2ull * p.Do * p.Ho * p.Wo * p.Cout;
    unsigned long long in_item = 0;
    for (int i = 0; i < p.n_src; ++i) {
        const unsigned long long b = 2ull * p.Di * p.Hi * p.Wi * p.src[i].C;
        in_item = b > in_item ? b : in_item;
    }
    if (out_item >= (1ull << 31) || in_item >= (1ull << 32) || (long long)p.Di * p.Hi >= (1 << 24) || p.Wi >= (1 << 24)) return false;
    if (zp_choose(p, o, c) || zr_choose(p, o, c)) return true;
    c = ConvChoice{};
    return row_choose(tp, o, c) || conv_choose_linear(p, o, c);
}

// Whether e4m3 operands stick (tp.c.fp8 on entry: the caller asks for them): only the stride-1 layers of 27 taps that the
// fp8 ZR kernel takes (the strided depth-shift kernel is fp16 only).  The choice sees the fp8 flag the launch will carry
// (the fp16-only six-row tiles); a layer the fp8 choice refuses is chosen again with fp16 operands.
bool conv_choose_fp8(ThinParams &tp, const ConvOverrides &o, ConvChoice &c) {
    ConvParams &p = tp.c;
    if (p.fp8 && !(p.kd * p.kh * p.kw == 27 && p.sd == 1 && p.sh == 1 && p.sw == 1)) p.fp8 = 0;
    bool ok = conv_choose(tp, o, c);
    if (p.fp8 && c.packing != FNN_PACK_ZR) { p.fp8 = 0; ok = conv_choose(tp, o, c); }
    return ok;
}

int launch_conv(const ThinParams &tp_in, const ConvChoice &c, hipStream_t st) {
    if (c.kernel == CK_ROW_STEM && tp_in.Y * tp_in.Z >= (1ll << 30)) {
        // the row form addresses the volume's planes with 32-bit offsets: a volume that large takes the tile form (the one
        // choice the call makes)
        ConvChoice t;
        return thin_choose(tp_in, t) ? launch_conv(tp_in, t, st) : -1;
    }
    fnn_note_kernel("%s", c.name);
    ThinParams tp = tp_in;
    ConvParams &p = tp.c;
    p.packing = c.packing; p.ksteps = c.ksteps; p.chunks = c.chunks; p.stats_slots = c.stats_slots;
    switch (c.kernel) {
        case CK_ZS: case CK_ZSP: case CK_ZSW: case CK_ZR: case CK_ZR8: case CK_ZQ12: case CK_ZR12: case CK_ZRW:
            return launch_conv3d_zr(p, c, st);
        case CK_ZP: case CK_ZPS: return launch_conv2d_zp(p, c, st);
        case CK_ROW: case CK_ROW_STEM: return launch_conv_row(tp, c, st);
        case CK_THIN: return launch_conv_thin(tp, c, st);
        case CK_PERSIST: return launch_persist(p, c, st);
        case CK_LDSK:
            if (c.t[1] == 2) {
                if (c.t[2] == 8) return c.t[0] == 2 ? launch_ldsk<2, 2, 8>(p, st) : launch_ldsk<1, 2, 8>(p, st);
                return c.t[0] == 2 ? launch_ldsk<2, 2, 16>(p, st) : launch_ldsk<1, 2, 16>(p, st);
            }
            if (c.t[0] == 1) return c.t[1] == 8 ? launch_ldsk<1, 8>(p, st) : launch_ldsk<1, 4>(p, st);
            return c.t[1] == 8 ? launch_ldsk<2, 8>(p, st) : launch_ldsk<2, 4>(p, st);
        case CK_S2: return launch_conv3d_s2(p, c, st);
        case CK_NB: return c.t[0] == 4 ? launch_conv_nb<4>(p, st) : c.t[0] == 2 ? launch_conv_nb<2>(p, st) : launch_conv_nb<1>(p, st);
    }
    return -1;
}
