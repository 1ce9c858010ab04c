// head.hip - the accumulate path's seg head (gfx950): 1x1x1 conv + Gaussian weighting + accumulation into the
// HBM-resident volume accumulators (SURVEY.md K6 + K7), the raw patch logits of the mirroring path, and the mirrored
// evaluations' mean -> accumulators (K9).  The gather path's form of the same arithmetic is gather.hip.
#include "act_load.h"
#include "output_common.h"

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
            const f32x4 b4 = a < nhb ? head_bias(p.bias, hb0 + a, q) : (f32x4){0.f, 0.f, 0.f, 0.f};
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
                    const f16x8 wf = head_frag(p.wpk, hb0 + hb, p.ksteps, ks, lane);
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
        for (int hb = 0; hb < 4; ++hb) bv[hb] = head_bias(p.bias, head_block(hb_first + hb, p.hblocks), q);
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
                aelem[i] = acc_voxel_of_patch(p, d, h, w) * p.HP + cb0 + grp_c * 8;
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
                for (int hb = 0; hb < 4; ++hb) wf[hb] = head_frag(p.wpk, head_block(hb_first + hb, p.hblocks), p.ksteps, ks, lane);
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
                aelem[rd][i] = acc_voxel_of_patch(p, d, h, w) * p.HP + cb0 + grp_c * 8;
                first[rd][i] = d >= p.fx && h >= p.fy && w >= p.fz;     // nobody has written this voxel yet
                graw[rd][i] = p.gauss[vv];                              // always a map (all ones without Gaussian weighting)
            }
        // first-visit voxels read one (hot) line of the patch's first voxel instead of their own: the load stays
        // unconditional (lesson 1 in DESIGN.md) and costs no HBM traffic; its value is discarded below
        const size_t dummy = acc_voxel_of_patch(p, 0, 0, 0) * p.HP + cb0 + grp_c * 8;
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
            const int hbc = head_block(hb_first + hb, p.hblocks);
            wf[hb] = head_frag(p.wpk, hbc, 1, 0, lane);
            bv[hb] = head_bias(p.bias, hbc, q);
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
    const size_t aelem = acc_voxel_of_patch(p, d, h, w) * p.HP;
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
