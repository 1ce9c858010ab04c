// conv_zr_common.h - what the depth-shift conv kernels share (conv3d_zr.hip: zr, zrw, zr12, zs, zsp, zsw, zr8; conv3d_zq.hip:
// zq12): the LDS layouts, the MFMA "B" operand's tap offsets, the k-loop of one chunk and the interleaved-cout epilogue.
#pragma once
#include "conv_common.h"

// ----------------------------------------------------------------------------
// LDS layouts: a kernel takes its offsets from its struct, its launcher the size - [image | weights | tail]
// ----------------------------------------------------------------------------
// conv3d_zr_kernel<NB, TD, TH> and conv3d_zrw_kernel<NB> (TD = 8, TH = 8): halo image [TD + 2][TH + 2][PW] voxels x 32 B,
// row pitch 12 = 4 (mod 8) voxels, halves swapped on odd rows; weights [NB][15][64 lanes][16 B].  No tail: the statistics'
// reduction floats reuse the image (zrw: the two unused voxel slots of every halo row).
template <int NB, int TD, int TH = 8>
struct ZrLds {
    static constexpr int PW = 12, PS = (TH + 2) * PW * 32;   // bytes per halo plane
    static constexpr int image = (TD + 2) * PS;               // no rounding: at TD = 4 the workgroup is 42 LDS granules (3 per CU)
    static constexpr int weights = NB * 15 * 1024;
    static constexpr int bytes() { return image + weights; }
};
// conv3d_zr12_kernel<TD> (NW = 9 waves) and conv3d_zq12_kernel (TD = 8, NW = 8): whole planes, halo [TD + 2][14][PW = 20];
// tail: the reduction floats [NW][32][2]
template <int TD, int NW>
struct Zr12Lds {
    static constexpr int PW = 20, PS = 14 * PW * 32;
    static constexpr int image = (TD + 2) * PS;
    static constexpr int weights = 2 * 15 * 1024;
    static constexpr int tail = NW * 32 * 2 * 4;
    static constexpr int bytes() { return image + weights + tail; }
};
// conv3d_zs_kernel<NB> (RED = false: the tail is the bias row, the reduction reuses the image) and conv3d_zsp_kernel /
// conv3d_zsw_kernel (RED = true: the reduction floats [4 waves][NB * 16][2]): halo [10][9][PW = 17], no swap
template <int NB, bool RED>
struct ZsLds {
    static constexpr int PW = 17, PS = 9 * PW * 32;
    static constexpr int image = (10 * PS + 1023) & ~1023;
    static constexpr int weights = NB * 15 * 1024;
    static constexpr int tail = RED ? 4 * NB * 16 * 2 * 4 : NB * 16 * 4;
    static constexpr int bytes() { return image + weights + tail; }
};
// conv3d_zr8_kernel<NB, TD>: [plane][row][8-channel half][24 slots of 8 B] (sub-row pitch SUB), weights at 8 B per lane;
// tail: [NB * 16] bias, then [NB * 16] output scales
template <int NB, int TD>
struct Zr8Lds {
    static constexpr int SUB = 192, PS = 10 * 2 * SUB;
    static constexpr int image = ((TD + 2) * PS + 1023) & ~1023;
    static constexpr int weights = NB * 15 * 512;
    static constexpr int tail = NB * 128;
    static constexpr int bytes() { return image + weights + tail; }
};

// ----------------------------------------------------------------------------
// MFMA "B" operand offsets
// ----------------------------------------------------------------------------
// lane = (voxel r of the wave's 16, k-group): k-group bit 1 picks the tap of the pair, bit 0 the 8-channel half.
// row_of_r(r), col_of_r(r): voxel r in the halo image at tap (0, 0) - its output position, doubled at in-plane stride 2;
// at(row, col, kh): the image's byte offset of (row, column, half).  Pair 4's second slot is padding: any finite data (its weights are 0;
// FNN_PACK_ZRP: tap 8).
template <class Row, class Col, class At>
static __device__ __forceinline__ void zr_tap_offsets(int (&toff)[5], int lane, Row row_of_r, Col col_of_r, At at) {
    const int r = lane & 15, hl = lane >> 5, kh = (lane >> 4) & 1;
#pragma unroll
    for (int pr = 0; pr < 5; ++pr) {
        const int tp = 2 * pr + hl < 9 ? 2 * pr + hl : 8;
        const int row = row_of_r(r) + tp / 3, col = col_of_r(r) + tp % 3;
        toff[pr] = at(row, col, kh);
    }
}
// the fp16 images: 32 B per voxel at row pitch PW, SWAP: halves swapped on odd rows; + base
template <int PW, bool SWAP, class Row, class Col>
static __device__ __forceinline__ void zr_tap_offsets(int (&toff)[5], int lane, Row row_of_r, Col col_of_r, int base = 0) {
    zr_tap_offsets(toff, lane, row_of_r, col_of_r,
                   [base](int row, int col, int kh) { return base + (row * PW + col) * 32 + ((SWAP ? kh ^ (row & 1) : kh) * 16); });
}

// ----------------------------------------------------------------------------
// k-loop
// ----------------------------------------------------------------------------
// One in-plane tap pair: the operand of halo plane j + dz (xf, read once) serves depth tap dz of output slice j - per dz
// NB weight reads ([NB][KS][64 lanes][16 B] at sW) for TDW x NB MFMAs.
template <int TDW, int NB, int KS>
static __device__ __forceinline__ void zr_pair_mfma(f32x4 (&acc)[TDW][NB], const f16x8 (&xf)[TDW + 2], const char *sW, int pr, int lane) {
#pragma unroll
    for (int dz = 0; dz < 3; ++dz) {
        f16x8 wf[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) wf[nb] = *(const f16x8 *)(sW + ((nb * KS + pr * 3 + dz) * 64 + lane) * 16);
#pragma unroll
        for (int j = 0; j < TDW; ++j)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
                acc[j][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nb], xf[j + dz], acc[j][nb], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);                        // keep the next pair's reads from being hoisted: registers
}
// A chunk's five tap pairs over the wave's TDW + 2 planes; plane_off(pl): byte offset of its plane pl (pl * PS, or the
// plane's slot in a ring)
template <int TDW, int NB, int KS, class PlaneOff>
static __device__ __forceinline__ void zr_kloop(f32x4 (&acc)[TDW][NB], const char *sA, const int (&toff)[5], const char *sW, int lane,
                                                PlaneOff plane_off) {
#pragma unroll
    for (int pr = 0; pr < 5; ++pr) {
        const char *bp = sA + toff[pr];
        f16x8 xf[TDW + 2];
#pragma unroll
        for (int pl = 0; pl < TDW + 2; ++pl) xf[pl] = *(const f16x8 *)(bp + plane_off(pl));
        zr_pair_mfma<TDW, NB, KS>(acc, xf, sW, pr, lane);
    }
}

// ----------------------------------------------------------------------------
// epilogue
// ----------------------------------------------------------------------------
// NB = 2 in the interleaved channel order of conv3d_pack_cout (lane quarter q holds channels q * 8 .. + 7): bias (after
// `osc` for the fp8 form), round to fp16, one 16-byte channels-last store per (voxel, lane), statistics as in tile_epilogue
// (conv_common.h).  The lane's voxels: (od0 + mb, oh, ow) for the TDW slices of acc.
typedef int fnn_i32x4 __attribute__((ext_vector_type(4)));
template <int TDW, bool BIAS = true>
static __device__ __forceinline__ void zr_epilogue_pair(const ConvParams &p, const f32x4 (&acc)[TDW][2], const float4 (&bv)[2],
                                                        int n, int od0, int oh, int ow, int cb0, int lane,
                                                        float (&t1)[2][4], float (&t2)[2][4]) {
    const int q = lane >> 4;
    const unsigned item_bytes = (unsigned)p.Do * p.Ho * p.Wo * p.Cout * 2;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(p.out + (size_t)n * (item_bytes >> 1), 0,
                                                                           item_bytes, 0x00020000);
    const unsigned ovs2 = (unsigned)FNN_OVS(p) * 2;
    const unsigned coff = (unsigned)(cb0 + (q >> 1)) * (unsigned)(FNN_OCS(p) * 2) + (unsigned)(q & 1) * 16;   // output layout: fnn_device.h
    const bool ok_hw = oh < p.Ho && ow < p.Wo;
    const f16x2 ones = {(f16)1.f, (f16)1.f};
#pragma unroll
    for (int mb = 0; mb < TDW; mb += 2) {
        f16x8 o[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int od = od0 + mb + h;
            const bool ok = ok_hw && od < p.Do;
            unsigned voff = ok ? (unsigned)((od * p.Ho + oh) * p.Wo + ow) * ovs2 + coff : 0x80000000u;
#ifdef FNN_TMODE
            if (p.tmode & 4) voff = 0x80000000u;
#endif
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                o[h][nb * 4 + 0] = (f16)(BIAS ? acc[mb + h][nb][0] + bv[nb].x : acc[mb + h][nb][0]);
                o[h][nb * 4 + 1] = (f16)(BIAS ? acc[mb + h][nb][1] + bv[nb].y : acc[mb + h][nb][1]);
                o[h][nb * 4 + 2] = (f16)(BIAS ? acc[mb + h][nb][2] + bv[nb].z : acc[mb + h][nb][2]);
                o[h][nb * 4 + 3] = (f16)(BIAS ? acc[mb + h][nb][3] + bv[nb].w : acc[mb + h][nb][3]);
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(fnn_i32x4, o[h]), rsrc, voff, 0, 0);
            if (!ok) o[h] = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f16x2 pr = {o[0][nb * 4 + j], o[1][nb * 4 + j]};
                t1[nb][j] = __builtin_amdgcn_fdot2(pr, ones, t1[nb][j], false);
                t2[nb][j] = __builtin_amdgcn_fdot2(pr, pr, t2[nb][j], false);
            }
    }
}
