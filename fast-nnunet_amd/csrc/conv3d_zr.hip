// conv3d_zr.hip - 3x3x3 stride-1 Conv3d with depth-shift operand reuse (gfx950).
//
// Same GEMM view and fusions as conv3d_lds_kernel (conv3d.hip): D[cout, voxel] = W[cout, k] X[k, voxel]
// on v_mfma_f32_16x16x32_f16, halo tile of one 16-channel chunk + that chunk's weight fragments in LDS,
// producer InstanceNorm + LeakyReLU applied while staging, own statistics in the epilogue.  What changes
// is who owns which voxels: a wave owns two h rows (16 voxels = one MFMA column block) in EVERY depth
// slice of the TD x 8 x 8 output tile.  The "B" fragment of halo plane p for an in-plane tap pair is then
// the operand of depth tap dz for output slice p - dz, for all three dz: it is read from LDS once and
// feeds 3 MFMAs per cout block.  Per (chunk, tap pair) a wave issues TD + 2 activation reads and 3 NB weight
// reads for 3 TD NB MFMAs - 0.33 LDS reads per MFMA at NB = 2, TD = 8 instead of 0.63 in the linear-tap
// kernels, which at 32 output channels were bound by LDS bandwidth, not by the matrix cores.
// Cost: the 9 in-plane taps pair up into 5 k-steps (one half padded) -> 30 tap slots instead of 27.  FNN_PACK_ZRP (TH = 8)
// removes the padding for pairs of chunks: the leftover tap 8 of chunk c (held in registers from chunk c's k-loop) and of
// chunk c + 1 share one k-step -> 27 k-steps per 32 channels.
//
// Replaces the same reference code as conv3d.hip (ConvDropoutNormReLU stacks,
// nnUNetDistillationTrainer.py:141-173).
#include "fnn_device.h"
#include "conv_common.h"
#include "conv_zr_common.h"
#include <type_traits>
#include <cstdlib>

// The depth-shift kernels (FNN_PACK_ZR: 15 k-steps, one statistics row per tile): 3x3x3 layers of depth stride 1 with
// enough workgroups to fill the chip - in-plane stride 2 on the ZS kernels, stride 1 on the ZR kernels.  false: the layer
// keeps the other kernels.
bool zr_choose(const ConvParams &p, const ConvOverrides &o, ConvChoice &c) {
    if (p.kd != 3 || p.kh != 3 || p.kw != 3 || p.sd != 1) return false;
    const int nblk = p.Cout / 16;
    const int plan_n = p.plan_N > 0 ? p.plan_N : p.N;
    c.packing = FNN_PACK_ZR; c.ksteps = 15; c.chunks = p.chunks;
    // conv3d_zr_kernel<NB, TD, 8> on two or more chunks takes the paired order (FNN_PACK_ZRP), decided from the shape before
    // the overrides: a layer of the <2, 10, 6> form's shape keeps FNN_PACK_ZR under both kernels (its bits are the 8 x 8 x 8
    // kernel's under FNN_NO_ZR6 - the tests compare them)
    bool zr6_shape = false;
    if (p.sh == 2 && p.sw == 2) {
        // in-plane stride 2: an even number of cout blocks, enough tiles (conv3d_zs_kernel below)
        if (p.fp8 || nblk % 2 != 0 || (long long)p.Di * p.Hi * p.Wi >= (1 << 23) || p.Do < 8) return false;
        const int tiles_d = (p.Do + 7) / 8, tiles_h = (p.Ho + 3) / 4, tiles_w = (p.Wo + 7) / 8, groups = nblk / 2;
        if ((long long)plan_n * tiles_d * tiles_h * tiles_w * (p.Cout / 32) < 768) return false;
        c.stats_slots = tiles_d * tiles_h * tiles_w;
        const bool persistent = p.chunks == 1 && p.n_src == 1 && plan_n * c.stats_slots >= 512 * 8;
        if (persistent && !o.no_zsw && tiles_d >= 4) {
            // single-chunk layers with at least four tiles along d: the walking form (round 4)
            const long long cols = (long long)plan_n * tiles_h * tiles_w * groups;
            int segs = 1;                                     // enough workgroups for several rounds of the chip's 512 slots, tiles permitting
            while (cols * segs < 8 * 512 && segs * 2 <= tiles_d / 2) segs *= 2;
            c.tps = (tiles_d + segs - 1) / segs;
            c.segs = (tiles_d + c.tps - 1) / c.tps;
            c.kernel = CK_ZSW;
            snprintf(c.name, sizeof c.name, "conv3d_zsw_kernel");
        } else if (persistent) {
            // single-chunk layers: the persistent form (two workgroups per CU over all cout groups)
            c.gx = 512 / groups < 8 ? 8 : 512 / groups;
            c.kernel = CK_ZSP;
            snprintf(c.name, sizeof c.name, "conv3d_zsp_kernel");
        } else {
            c.kernel = CK_ZS; c.t[0] = 2;
            snprintf(c.name, sizeof c.name, "conv3d_zs_kernel<2>");
        }
        return true;
    }
    if (p.sh != 1 || p.sw != 1) return false;
    const long long vox = (long long)p.Do * p.Ho * p.Wo;                            // (stride 1: the input's size too)
    if (vox >= (1 << 23)) return false;                                             // 24-bit voxel index arithmetic in the kernels
    // the staging's zero padding is a buffer offset of 0x80000000 that the range check must refuse: every source's batch
    // item (and the output's) stays below 2^31 bytes - bounded here by all input channels together
    if (vox * 32 * (p.chunks > 0 ? p.chunks : 1) >= (1ll << 31) || vox * 2 * p.Cout >= (1ll << 31)) return false;
    const int nb = nblk % 2 == 0 ? 2 : 1;
    const int th = (p.Ho + 7) / 8, tw = (p.Wo + 7) / 8;
    // planes of at most 6 x 8 voxels in a layer whose depth is a multiple of 10 (the 160-channel stages of the benchmark net:
    // 20 x 6 x 6): tiles of 10 x 6 x 8 on three waves (conv3d_zr_kernel<2, 10, 6>) - 75 % of the tile's columns and all of its
    // depth are output voxels (8 x 8 x 8 tiles: 47 %)
    zr6_shape = nb == 2 && !p.fp8 && p.Ho <= 6 && p.Wo <= 8 && p.Do >= 10 && p.Do % 10 == 0 &&
                (long long)plan_n * (p.Do / 10) * (nblk / 2) >= 160;
    if (zr6_shape && !o.no_zr6) {
        c.stats_slots = ((p.Do + 9) / 10) * th * tw;
        c.kernel = CK_ZR; c.t[0] = 2; c.t[1] = 10; c.t[2] = 6;
        snprintf(c.name, sizeof c.name, "conv3d_zr_kernel<%d,%d,%d>", 2, 10, 6);
        return true;
    }
    // one round of 512 slots at TD = 8 beats two of 768 at TD = 4 (stage 4: 70 -> 64 us)
    int td = 8;
    while (td >= 4 && (p.Do < td || (long long)plan_n * ((p.Do + td - 1) / td) * th * tw * (nblk / nb) < o.zr_min_wgs)) td -= 4;
    if (td < 4) return false;
    c.stats_slots = ((p.Do + td - 1) / td) * th * tw;
    c.t[0] = nb; c.t[1] = td;
    if (p.fp8) {
        c.kernel = CK_ZR8;
        snprintf(c.name, sizeof c.name, "conv3d_zr8_kernel<%d,%d>", nb, td);
    } else if (nb == 2 && !o.no_zq12 && conv3d_zq12_fits(p, c.stats_slots)) {
        // planes of 9 .. 12 x 9 .. 12 voxels (two half-empty 8 x 8 tiles per axis): whole planes per tile.  Round 5: 8 x 12 x 12
        // tiles, eight balanced waves (conv3d_zq.hip)
        c.kernel = CK_ZQ12;
        snprintf(c.name, sizeof c.name, "conv3d_zq12_kernel");
    } else if (nb == 2 && p.Ho > 8 && p.Ho <= 12 && p.Wo > 8 && p.Wo <= 12 && c.stats_slots >= (p.Do + 3) / 4) {
        c.kernel = CK_ZR12; c.t[0] = 4;                                          // (TD = 6: 60 B of scratch, -1.5 %; TD = 8: 140-224 B, -3 %)
        snprintf(c.name, sizeof c.name, "conv3d_zr12_kernel<%d>", 4);
    } else if (p.chunks == 1 && td == 8 && (p.Do + 7) / 8 >= 4) {
        // one chunk (Cin <= 16) and at least four tiles along d: the walking form
        const int tiles_d = (p.Do + 7) / 8;
        const long long cols = (long long)plan_n * th * tw * (nblk / nb);
        int segs = 1;                                         // enough workgroups for two rounds of the chip's slots, tiles permitting
        while (cols * segs < 2 * 768 && segs * 2 <= tiles_d / 2) segs *= 2;
        c.tps = (tiles_d + segs - 1) / segs;
        c.segs = (tiles_d + c.tps - 1) / c.tps;
        c.kernel = CK_ZRW;
        snprintf(c.name, sizeof c.name, "conv3d_zrw_kernel<%d>", nb);
    } else {
        c.kernel = CK_ZR;
        if (p.chunks >= 2 && !zr6_shape && !o.no_zrp) c.packing = FNN_PACK_ZRP;
        snprintf(c.name, sizeof c.name, "conv3d_zr_kernel<%d,%d>", nb, td);
    }
    return true;
}

// Staging (round 3): a thread owns one COLUMN of the halo - (row zh, column zw, 8-channel half cg), 200 of the 256
// threads - and walks the TD + 2 planes.  Everything that used to be a per-element table (16 registers and ~35 VALU
// instructions per element to build: 43 % of the kernel's vector instructions sat in front of the first load) is now
// either one per-thread constant (the in-plane byte offset; 0x80000000 where the column lies outside the tensor: the
// buffer load's range check returns zeros without touching memory), a scalar per plane (the plane's byte offset as the
// load's soffset, clamped into the tensor; a plane outside it is not written - its LDS image was zeroed once) or an
// immediate (LDS offsets).  The weights' two cout blocks get a buffer descriptor each whose num_records ends the block's
// 15 k-steps: fragment element tid + 256 u needs no per-lane address either.  The bias is the accumulators' initial value.
typedef unsigned fnn_u32x4v __attribute__((ext_vector_type(4)));
// TH = 8: the tile's rows, four waves.  TH = 6 (round 5, NB = 2): planes of at most 6 rows - three waves, a halo of 8 rows, the
// depth the register file allows (TD = 10: 20-deep layers in two tiles) - for the 160-channel stages of a 96 x 96 in-plane patch
// (20 x 6 x 6), where 8 x 8 x 8 tiles are filled to 47 % and their fourth wave multiplies rows that do not exist.
template <int NB, int TD, int TH = 8>
__global__ __launch_bounds__(TH * 32, 2) void conv3d_zr_kernel(const ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    FNN_STAMP_DECL
    FNN_STAMP();                                              // 0: entry
    constexpr int NT = TH * 32;                               // threads: one wave per pair of tile rows
    using L = ZrLds<NB, TD, TH>;
    constexpr int IH = TH + 2, IW = 10, PW = L::PW, ID = TD + 2;   // halo tile
    constexpr int PS = L::PS, ABYTES = L::image;
    constexpr int KS = 15;
    constexpr int WB = KS * 64;                               // 16-byte weight elements per cout block and chunk
    constexpr int WPB = (WB + NT - 1) / NT;                   // loads per thread and cout block (256 threads: the last one by waves 0 .. 2 only)
    static_assert(WB - (WPB - 1) * NT == 192, "the last weight element group covers exactly waves 0 .. 2");

    // XCD-aware, bijective remap (blocks b and b + 8 share an XCD)
    int t = __builtin_amdgcn_readfirstlane(fnn_xcd_tile(gridDim.x, blockIdx.x));
    const int tw = __builtin_amdgcn_readfirstlane(t % p.tiles_w); t = __builtin_amdgcn_readfirstlane(t / p.tiles_w);
    const int th = __builtin_amdgcn_readfirstlane(t % p.tiles_h); t = __builtin_amdgcn_readfirstlane(t / p.tiles_h);
    const int td = __builtin_amdgcn_readfirstlane(t % p.tiles_d);
    const int n = __builtin_amdgcn_readfirstlane(t / p.tiles_d);
    const int cb0 = blockIdx.y * NB;
    const int od0 = td * TD, oh0 = th * 8, ow0 = tw * 8;

    char *sA = smem;                                          // halo image: [ID][IH][PW] voxels x 32 B, halves swapped on odd rows
    char *sW = smem + ABYTES;                                 // [NB][15][64 lanes][16 B]

    // ---- this thread's halo column
    const int col = tid >> 1, cg = tid & 1;
    const int zh = (col * 205) >> 11, zw = col - zh * IW;     // col / 10 for col < 128
    const bool has_col = tid < 2 * IH * IW;
    const int gh = oh0 - 1 + zh, gw = ow0 - 1 + zw;
    const bool ok_hw = has_col & ((unsigned)gh < (unsigned)p.Hi) & ((unsigned)gw < (unsigned)p.Wi);
    const int hw_lin = __mul24(gh, p.Wi) + gw;
    const int ldso0 = (zh * PW + zw) * 32 + ((cg ^ (zh & 1)) * 16);
    const int wlds = ABYTES + tid * 16;
    // planes of the halo that lie inside the tensor (bit u), and the clamped plane numbers
    unsigned pmask = (1u << ID) - 1;                          // (scalar arithmetic: a plane test is one s_bitcmp)
    if (od0 == 0) pmask &= ~1u;
    {
        const int over = od0 + TD + 1 - p.Di;                 // planes beyond the last one
        if (over > 0) pmask &= (1u << (ID - over)) - 1;
    }
    pmask = __builtin_amdgcn_readfirstlane(pmask);

    f32x4 acc[TD][NB];
    fnn_u32x4v xr[ID], wr[NB][WPB];
    // FNN_PACK_ZRP (TH = 8 only: the 6-row form has no registers to spare): chunk 2 i's leftover-tap operands, read in its
    // k-loop, wait here for chunk 2 i + 1's (lanes of k-half 1 take that chunk's, k-half 0 keep these)
    constexpr bool PAIR = TH == 8;
    const bool paired = PAIR && p.packing == FNN_PACK_ZRP;
    f16x8 xl[PAIR ? ID : 1];
#ifdef FNN_NORM_FP32
    float scu[16], shu[16];                                   // the chunk's scale / shift rows: wave-uniform -> scalar loads
#else
    fnn_u32x4v ssv[2];                                        // this thread's 8 scales and 8 shifts in fp16 (SrcDesc::ssh): two 16-byte loads
#endif
    float slope_next = 1.f;
#ifdef FNN_TMODE
    bool first_chunk = true;
#endif

    // The chunk's loads in five slices, one per tap pair of the k-loop: issued in one block the 18 wave-wide loads of
    // every wave of the CU queue up in the texture-address path and the MFMAs behind them cannot issue (in-order waves).
    __amdgpu_buffer_rsrc_t rx, rw[NB];
    unsigned voff = 0x80000000u, plane_bytes = 0;
    auto prep = [&](int ch) {
        const int c_glob = ch * 16;
        const int s = (c_glob < p.src[0].C) ? 0 : 1;
        const int c_uni = c_glob - (s ? p.src[0].C : 0);
        const int sC = p.src[s].C;
        const int vs = FNN_VS(p.src[s]);                      // activation layout: fnn_device.h, SrcDesc
        const unsigned item_bytes = (unsigned)p.Di * p.Hi * p.Wi * sC * 2;
        const f16 *sp = p.src[s].ptr + (size_t)n * (item_bytes >> 1) + (c_uni >> 4) * FNN_CS(p.src[s]);
        rx = __builtin_amdgcn_make_buffer_rsrc((void *)sp, 0, item_bytes, 0x00020000);
        slope_next = p.src[s].slope;
#ifdef FNN_NORM_FP32
        const float *qs, *qh;
        fnn_ss_rows(p.src[s].ss, sC, n, c_uni, p.ident_ss, qs, qh);
#pragma unroll
        for (int j = 0; j < 16; ++j) { scu[j] = qs[j]; shu[j] = qh[j]; }
#else
        {
            const fnn_u32x4v *qv = (const fnn_u32x4v *)(fnn_ssh_rows(p.src[s].ssh, sC, n, c_uni, p.ident_ssh) + cg * 16);
            ssv[0] = qv[0]; ssv[1] = qv[1];
        }
#endif
        voff = ok_hw ? (unsigned)hw_lin * (unsigned)(vs * 2) + cg * 16 : 0x80000000u;
        plane_bytes = (unsigned)p.Hi * p.Wi * vs * 2;
        // the first chunk of a pair: its k-steps 12 .. 14 are zeros (the shared k-steps are the second chunk's) - the range
        // check returns them without traffic
        const int wbytes = paired && ch % 2 == 0 && ch + 1 < p.chunks ? 12 * 64 * 16 : WB * 16;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const f16 *wp = p.wpk + ((size_t)((cb0 + nb) * p.chunks + ch) * WB) * 8;
            rw[nb] = __builtin_amdgcn_make_buffer_rsrc((void *)wp, 0, wbytes, 0x00020000);
        }
    };
#ifndef FNN_ZR_SLICES
#define FNN_ZR_SLICES 5
#endif
    constexpr int SL = FNN_ZR_SLICES;
    auto load_part = [&](int part) {                          // part 0 .. SL - 1
#pragma unroll
        for (int u = 0; u < ID; ++u) {
            if (u * SL / ID != part) continue;
            int gd = od0 - 1 + u;
            gd = gd < 0 ? 0 : (gd >= p.Di ? p.Di - 1 : gd);   // scalar; a clamped plane's image is zeroed in commit()
            xr[u] = __builtin_bit_cast(fnn_u32x4v, __builtin_amdgcn_raw_buffer_load_b128(rx, voff, (unsigned)gd * plane_bytes, 0));
        }
#ifdef FNN_TMODE
        if ((p.tmode & 8) && !first_chunk) return;            // proxy: no weight traffic after the first chunk
#endif
#pragma unroll
        for (int e = 0; e < NB * WPB; ++e) {                  // element tid + 256 u of block nb; beyond the block: range check, zeros, no traffic
            if (e * SL / (NB * WPB) != part) continue;
            const int nb = e / WPB, u = e % WPB;
            wr[nb][u] = __builtin_bit_cast(fnn_u32x4v, __builtin_amdgcn_raw_buffer_load_b128(rw[nb], tid * 16, u * (NT * 16), 0));
        }
    };
    auto commit = [&]() {
        const f16 slope_h = (f16)slope_next;
#ifdef FNN_NORM_FP32
        float sc[8], sh[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {                         // a column outside the tensor: 0 * 0 + 0 = the conv's zero padding
            sc[j] = ok_hw ? (cg ? scu[8 + j] : scu[j]) : 0.f;
            sh[j] = ok_hw ? (cg ? shu[8 + j] : shu[j]) : 0.f;
        }
#else
        // scale and shift in fp16 (fnn_norm_leaky8, conv_common.h).  A column outside the tensor: 0 * 0 + 0 = the conv's zero padding.
        const fnn_u32x4v zero4 = {0u, 0u, 0u, 0u};
        const f16x8 sc = __builtin_bit_cast(f16x8, ok_hw ? ssv[0] : zero4), sh = __builtin_bit_cast(f16x8, ok_hw ? ssv[1] : zero4);
#endif
        if (has_col) {
#pragma unroll
            for (int u = 0; u < ID; ++u)
                *(f16x8 *)(sA + ldso0 + u * PS) = fnn_norm_leaky8(__builtin_bit_cast(f16x8, xr[u]), sc, sh, slope_h);
            if (pmask != (1u << ID) - 1) {                    // border tiles along d: planes outside the tensor (a clamped plane's data were written above)
                unsigned pm = pmask;
#ifdef FNN_NORM_FP32
                pm = __builtin_amdgcn_readfirstlane(pm);      // (in this build pmask arrives here in a VGPR: "illegal VGPR to SGPR copy")
#endif
                asm volatile("" : "+s"(pm));                  // (hoisted out of the chunk loop the tests become lane masks: 20 SGPRs, spilled)
#pragma unroll
                for (int u = 0; u < ID; ++u)
                    if (!((pm >> u) & 1)) *(f16x8 *)(sA + ldso0 + u * PS) = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
            }
        }
#ifdef FNN_TMODE
        if ((p.tmode & 8) && !first_chunk) return;
#endif
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int u = 0; u < WPB; ++u)
                if (u + 1 < WPB || wave < 3) *(fnn_u32x4v *)(smem + wlds + (nb * WB + u * NT) * 16) = wr[nb][u];
    };
    int toff[5];                                              // filled in after the first loads have left
    const bool khalf1 = lane >= 32;                           // MFMA "B" lanes of k 16 .. 31 (the second tap of a pair)
    // MODE (wave-uniform, one k-loop copy each): 0 = the padded order; 1 = first chunk of a pair: tap pair 4's operands go to
    // xl, no MFMAs; 2 = second chunk of a pair: the shared k-steps FIRST - k-half 0 from xl (the first chunk's tap 8), k-half 1
    // this chunk's - so that xl is dead before the other pairs' operands and the next chunk's prefetch registers are live
    // (kept live through them it spilled)
    auto kloop = [&](bool prefetch, auto mode_c) __attribute__((always_inline)) {
        constexpr int MODE = decltype(mode_c)::value;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int pr = MODE == 2 ? (i + 4) % 5 : i;
            if (prefetch && i < SL) load_part(i);
            const char *bp = sA + toff[pr];
            if (MODE == 1 && pr == 4) {
#pragma unroll
                for (int pl = 0; pl < ID; ++pl) xl[pl] = *(const f16x8 *)(bp + pl * PS);
                break;
            }
            f16x8 xf[ID];
#pragma unroll
            for (int pl = 0; pl < ID; ++pl) xf[pl] = *(const f16x8 *)(bp + pl * PS);
            if (MODE == 2 && pr == 4) {
#pragma unroll
                for (int pl = 0; pl < ID; ++pl) xf[pl] = khalf1 ? xf[pl] : xl[pl];
            }
            zr_pair_mfma<TD, NB, KS>(acc, xf, sW, pr, lane);
        }
    };
    prep(0);
#pragma unroll
    for (int part = 0; part < SL; ++part) load_part(part);
    __builtin_amdgcn_sched_barrier(0);                        // the loads leave first; the rest of the set-up runs under them
    FNN_STAMP();                                              // 1: first loads issued
    // the bias is where the accumulators start (lane = channels (lane >> 4) * 8 + nb * 4 .. + 3 of its block pair in the
    // interleaved order of conv3d_pack_cout at NB = 2, (lane >> 4) * 4 .. + 3 of block nb otherwise)
    {
        f32x4 b0[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
            b0[nb] = *(const f32x4 *)(p.bias + cb0 * 16 + (NB == 2 ? (lane >> 4) * 8 + nb * 4 : nb * 16 + (lane >> 4) * 4));
#pragma unroll
        for (int j = 0; j < TD; ++j)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[j][nb] = b0[nb];
    }
    // MFMA "B" operand: lane = (voxel r of the wave's two rows, k-group): k-group bit 1 picks the tap of the pair,
    // bit 0 the 8-channel half.  (zr_tap_offsets' text, kept here: through the helper <1, 8> took 168 instead of 165 VGPRs)
    {
        const int r = lane & 15, hl = lane >> 5, kh = (lane >> 4) & 1;
#pragma unroll
        for (int pr = 0; pr < 5; ++pr) {
            const int tp = 2 * pr + hl < 9 ? 2 * pr + hl : 8;   // padded slot: any finite data (its weights are 0); FNN_PACK_ZRP: tap 8
            const int row = 2 * wave + (r >> 3) + tp / 3, col2 = (r & 7) + tp % 3;
            toff[pr] = (row * PW + col2) * 32 + ((kh ^ (row & 1)) * 16);
        }
    }

    commit();
#ifdef FNN_TMODE
    first_chunk = false;
#endif
    __syncthreads();
    FNN_STAMP();                                              // 2: first chunk staged
    // the last chunk is peeled off so that the wait for the prefetch sits on an unconditional path (see conv3d_lds_kernel)
    using M0 = std::integral_constant<int, 0>;
    using M1 = std::integral_constant<int, 1>;
    using M2 = std::integral_constant<int, 2>;
    auto next_chunk = [&](int ch, auto mode_c) __attribute__((always_inline)) {   // k-loop of chunk ch, then stage ch + 1
        prep(ch + 1);
        kloop(true, mode_c);                                  // global loads stay in flight during the MFMAs
        FNN_STAMP();                                          // k-loop done
        __syncthreads();                                      // every wave is done reading this chunk
        commit();
        __syncthreads();
        FNN_STAMP();                                          // next chunk staged
    };
    if (PAIR && paired) {
        // one pair per iteration, straight-line: with the two orders' k-loops behind a branch in one loop body the
        // prefetch registers of both arms spilled
        int ch = 0;
        for (; ch + 2 < p.chunks; ch += 2) {
            next_chunk(ch, M1{});
            next_chunk(ch + 1, M2{});
        }
        if (ch + 1 < p.chunks) {
            next_chunk(ch, M1{});
            kloop(false, M2{});
        } else {
            kloop(false, M0{});                               // an unpaired last chunk: the padded order
        }
    } else {
        for (int ch = 0; ch + 1 < p.chunks; ++ch) next_chunk(ch, M0{});
        kloop(false, M0{});
    }
    FNN_STAMP();
    __syncthreads();

    // ---- epilogue: fp16 store, statistics (the bias is in the accumulators)
    {
        float4 bv[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) bv[nb] = make_float4(0.f, 0.f, 0.f, 0.f);
        float t1[NB][4], t2[NB][4];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int j = 0; j < 4; ++j) { t1[nb][j] = 0.f; t2[nb][j] = 0.f; }
        if constexpr (NB == 2) zr_epilogue_pair<TD, false>(p, acc, bv, n, od0, oh0 + 2 * wave + ((lane & 15) >> 3), ow0 + (lane & 7), cb0, lane, t1, t2);
        else tile_epilogue<NB, TD, true, false>(p, acc, bv, n, od0, oh0, ow0, cb0, wave, lane, t1, t2);
        if (p.stats_out) stats_to_global<NB, true, NB == 2, TH / 2>(p, t1, t2, (float *)smem, n, cb0, wave, lane, tid, (td * p.tiles_h + th) * p.tiles_w + tw);
    }
    FNN_STAMP();                                              // epilogue done
    FNN_STAMP_FLUSH(p.dbg);
}

// (Round 4's role-split form of this kernel - conv3d_zrs_kernel: one 768-thread workgroup per CU, four multiplying and eight
// staging waves, -10.6 % cycles per tile at -9 % clock - was an opt-in experiment behind FNN_ZRS; its last step-level A-B in
// round 5 (3516 / 3512 vs 3507 / 3500 patches/s) confirmed 0 +- 0.4 %, and it is gone: DESIGN.md 7.0 keeps the finding, the
// source is in the history at commit "conv3d_zq12_kernel" and before.)

// ----------------------------------------------------------------------------
// single-chunk layers (Cin <= 16): the same kernel WALKING along d (round 3)
// ----------------------------------------------------------------------------
// A 16 -> 16 (or 16 -> 32) 3x3x3 layer at full resolution - stage 0 of every isotropic network: 38 % of the 128^3
// student's time, 22 % of the ResEnc student's - is one chunk per tile: conv3d_zr_kernel has nothing to prefetch behind
// (load, wait, stage, 120 MFMAs per wave, store) and re-reads the chunk's 15 KB of weights and two of its ten halo planes
// for every tile.  Here a workgroup owns an 8 x 8 in-plane window and walks `tps` consecutive d-tiles: the weights are
// staged once, the halo image is a RING of ten planes - a tile brings its eight new planes, the last two of its
// predecessor stay where they are - and the next tile's planes are in flight during the current tile's k-loop.  Same
// per-tile arithmetic, tile decomposition and statistics rows as conv3d_zr_kernel<NB, 8>: bit-identical results.
template <int NB>
__global__ __launch_bounds__(256, NB == 1 ? 3 : 2) void conv3d_zrw_kernel(const ConvParams p, const int segs, const int tps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    using L = ZrLds<NB, 8>;
    constexpr int TD = 8, IH = 10, IW = 10, PW = L::PW, ID = TD + 2;
    constexpr int PS = L::PS, ABYTES = L::image, KS = 15, WB = KS * 64, WPB = (WB + 255) / 256;

    int t = __builtin_amdgcn_readfirstlane(fnn_xcd_tile(gridDim.x, blockIdx.x));
    const int tw = __builtin_amdgcn_readfirstlane(t % p.tiles_w); t = __builtin_amdgcn_readfirstlane(t / p.tiles_w);
    const int th = __builtin_amdgcn_readfirstlane(t % p.tiles_h); t = __builtin_amdgcn_readfirstlane(t / p.tiles_h);
    const int seg = __builtin_amdgcn_readfirstlane(t % segs);
    const int n = __builtin_amdgcn_readfirstlane(t / segs);
    const int td0 = seg * tps, td1 = td0 + tps < p.tiles_d ? td0 + tps : p.tiles_d;
    if (td0 >= td1) return;
    const int cb0 = blockIdx.y * NB;
    const int oh0 = th * 8, ow0 = tw * 8;

    char *sA = smem;                                          // ring of ID halo planes: plane 8 td0 - 1 + k sits in slot k % ID
    char *sW = smem + ABYTES;                                 // [NB][15][64 lanes][16 B], resident
    // the statistics' reduction floats (4 waves x NB x 16 channels x 2) live in the two unused voxel slots behind the ten
    // used ones of every halo row (pitch 12): 16 floats per row - a kilobyte of their own would cost the third workgroup per CU
    auto sred_at = [&](int i) { const int k = i >> 4; return (float *)(sA + (k / IH) * PS + ((k % IH) * PW + IW) * 32) + (i & 15); };

    const int col = tid >> 1, cg = tid & 1;
    const int zh = (col * 205) >> 11, zw = col - zh * IW;
    const bool has_col = tid < 2 * IH * IW;
    const int gh = oh0 - 1 + zh, gw = ow0 - 1 + zw;
    const bool ok_hw = has_col & ((unsigned)gh < (unsigned)p.Hi) & ((unsigned)gw < (unsigned)p.Wi);
    const int hw_lin = __mul24(gh, p.Wi) + gw;
    const int ldso0 = (zh * PW + zw) * 32 + ((cg ^ (zh & 1)) * 16);

    // the one chunk: source 0, channels 0 .. 15 - descriptors, offsets and the normalisation are the walk's constants
    const int sC = p.src[0].C, vs = FNN_VS(p.src[0]);
    const unsigned item_bytes = (unsigned)p.Di * p.Hi * p.Wi * sC * 2;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void *)(p.src[0].ptr + (size_t)n * (item_bytes >> 1)), 0, item_bytes, 0x00020000);
    const unsigned voff = ok_hw ? (unsigned)hw_lin * (unsigned)(vs * 2) + cg * 16 : 0x80000000u;
    const unsigned plane_bytes = (unsigned)p.Hi * p.Wi * vs * 2;
    const f16 slope_h = (f16)p.src[0].slope;
#ifdef FNN_NORM_FP32
    float sc[8], sh[8];
    {
        const float *qs, *qh;
        fnn_ss_rows(p.src[0].ss, sC, n, 0, p.ident_ss, qs, qh);
#pragma unroll
        for (int j = 0; j < 8; ++j) { sc[j] = ok_hw ? qs[cg * 8 + j] : 0.f; sh[j] = ok_hw ? qh[cg * 8 + j] : 0.f; }
    }
#else
    f16x8 sc, sh;
    {
        const fnn_u32x4v *qv = (const fnn_u32x4v *)(fnn_ssh_rows(p.src[0].ssh, sC, n, 0, p.ident_ssh) + cg * 16);
        const fnn_u32x4v zero4 = {0u, 0u, 0u, 0u};
        sc = __builtin_bit_cast(f16x8, ok_hw ? qv[0] : zero4); sh = __builtin_bit_cast(f16x8, ok_hw ? qv[1] : zero4);
    }
#endif

    fnn_u32x4v xr[ID];
    auto load_planes = [&](int td, int u0) {                  // the planes u0 .. 9 of tile td: 8 td - 1 + u, clamped (see stage())
#pragma unroll
        for (int u = 0; u < ID; ++u) {
            if (u < u0) continue;
            int gd = td * TD - 1 + u;
            gd = gd < 0 ? 0 : (gd >= p.Di ? p.Di - 1 : gd);
            xr[u] = __builtin_bit_cast(fnn_u32x4v, __builtin_amdgcn_raw_buffer_load_b128(rx, voff, (unsigned)gd * plane_bytes, 0));
        }
    };
    auto stage = [&](int td, int u0) {                        // normalise + LeakyReLU, into the planes' ring slots; planes outside the tensor: zeros
        if (!has_col) return;
        const int k0 = (td - td0) * TD;
#pragma unroll
        for (int u = 0; u < ID; ++u) {
            if (u < u0) continue;
            f16x8 o = fnn_norm_leaky8(__builtin_bit_cast(f16x8, xr[u]), sc, sh, slope_h);
            const int gd = td * TD - 1 + u;                   // (scalar)
            if ((unsigned)gd >= (unsigned)p.Di) o = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
            *(f16x8 *)(sA + ldso0 + ((k0 + u) % ID) * PS) = o;
        }
    };
    int toff[5];
    f32x4 acc[TD][NB];
    auto kloop = [&](int td) {
        const int k0 = (td - td0) * TD;
        int roff[ID];                                         // (scalars) where the tile's ten planes sit in the ring
#pragma unroll
        for (int pl = 0; pl < ID; ++pl) roff[pl] = ((k0 + pl) % ID) * PS;
        zr_kloop<TD, NB, KS>(acc, sA, toff, sW, lane, [&](int pl) { return roff[pl]; });
    };

    // ---- prologue: the first tile's ten planes and the weights
    load_planes(td0, 0);
    fnn_u32x4v wr[NB][WPB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const f16 *wp = p.wpk + ((size_t)((cb0 + nb) * p.chunks) * WB) * 8;
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void *)wp, 0, WB * 16, 0x00020000);
#pragma unroll
        for (int u = 0; u < WPB; ++u) wr[nb][u] = __builtin_bit_cast(fnn_u32x4v, __builtin_amdgcn_raw_buffer_load_b128(rw, tid * 16, u * 4096, 0));
    }
    f32x4 b0[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
        b0[nb] = *(const f32x4 *)(p.bias + cb0 * 16 + (NB == 2 ? (lane >> 4) * 8 + nb * 4 : nb * 16 + (lane >> 4) * 4));
    zr_tap_offsets<PW, true>(toff, lane, [=](int r) { return 2 * wave + (r >> 3); }, [](int r) { return r & 7; });
    stage(td0, 0);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int u = 0; u < WPB; ++u)
            if (u + 1 < WPB || wave < 3) *(fnn_u32x4v *)(sW + ((nb * WB + u * 256) + tid) * 16) = wr[nb][u];
    __syncthreads();

    auto finish = [&](int td) {                               // fp16 stores + the tile's statistics row (the bias is in the accumulators)
        float4 bv[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) bv[nb] = make_float4(0.f, 0.f, 0.f, 0.f);
        float t1[NB][4], t2[NB][4];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int j = 0; j < 4; ++j) { t1[nb][j] = 0.f; t2[nb][j] = 0.f; }
        if constexpr (NB == 2) zr_epilogue_pair<TD, false>(p, acc, bv, n, td * TD, oh0 + 2 * wave + ((lane & 15) >> 3), ow0 + (lane & 7), cb0, lane, t1, t2);
        else tile_epilogue<NB, TD, true, false>(p, acc, bv, n, td * TD, oh0, ow0, cb0, wave, lane, t1, t2);
        if (p.stats_out) stats_to_global_at<NB, true, NB == 2>(p, t1, t2, sred_at, n, cb0, wave, lane, tid, (td * p.tiles_h + th) * p.tiles_w + tw);
        else __syncthreads();
    };
    // ---- the walk: the last tile is peeled off (nothing to prefetch behind it)
    for (int td = td0; td + 1 < td1; ++td) {
#pragma unroll
        for (int j = 0; j < TD; ++j)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[j][nb] = b0[nb];
        load_planes(td + 1, 2);                               // eight new planes, in flight during the MFMAs
        kloop(td);
        __syncthreads();                                      // every wave is done with this tile's planes
        stage(td + 1, 2);                                     // over the slots of this tile's first eight planes
        finish(td);                                           // (its barrier also publishes the staged planes)
    }
#pragma unroll
    for (int j = 0; j < TD; ++j)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[j][nb] = b0[nb];
    kloop(td1 - 1);
    __syncthreads();
    finish(td1 - 1);
}

// ----------------------------------------------------------------------------
// whole 12 x 12 planes per tile (the 128-channel stage of a 96 x 96 in-plane patch)
// ----------------------------------------------------------------------------
// 8 x 8 in-plane tiles cover a 12 x 12 plane with four tiles that are filled to 56 %: the MFMAs of the empty columns are
// wasted and a 10 x 10 x 10 halo is staged for 288 outputs (3.5 halo voxels per output; with 128 output channels once per
// 32 of them).  Here the tile is TD x 12 x 12: nine waves (576 threads), each the owner of one 4 x 4 column block in
// every depth slice - the depth-shift reuse of conv3d_zr_kernel unchanged (0.33 LDS reads per MFMA) - over a halo of
// (TD + 2) x 14 x 14 voxels: 1.7 halo voxels per output, every MFMA column a real voxel, and the chunk's 30 KB of weight
// fragments serve 1152 outputs instead of 288.  LDS image: row pitch 20 voxels (4 mod 8) with the channel halves
// swapped on odd rows: the 16 lanes of a ds_read_b128 group hold rows 0 and 3 of the block in one half and rows 1 and 2
// in the other - 16 different slots.  One workgroup per CU (120 KB of LDS); a SIMD holds two or three of its waves.
// Same weights (FNN_PACK_ZR, interleaved cout order), arithmetic and statistics rows (one per tile) as
// conv3d_zr_kernel; the sums of a statistics row are formed over other voxel groups: fp16-resolution differences.
template <int TD>
__global__ __launch_bounds__(576, 1) void conv3d_zr12_kernel(const ConvParams p) {
    constexpr int NB = 2, NT = 576;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    using L = Zr12Lds<TD, 9>;
    constexpr int IH = 14, IW = 14, PW = L::PW, ID = TD + 2;
    constexpr int PS = L::PS, ABYTES = L::image;
    constexpr int KS = 15;
    constexpr int IELEM = ID * IH * IW * 2;
    constexpr int PF = (IELEM + NT - 1) / NT;
    constexpr int WTOT = NB * KS * 64;
    constexpr int WPF = (WTOT + NT - 1) / NT;

    const int td = blockIdx.x % p.tiles_d, n = blockIdx.x / p.tiles_d;
    const int cb0 = blockIdx.y * NB;
    const int od0 = td * TD;
    const int bh = wave / 3, bw = wave - bh * 3;                      // this wave's 4 x 4 block of the plane

    char *sA = smem;
    char *sW = smem + ABYTES;
    float *sRed = (float *)(sW + L::weights);                 // [9 waves][32][2]

    const int cg = tid & 1;
    int offv[PF], ldso[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const int idx = tid + u * NT;
        const int v = idx >> 1;
        const int zd = v / (IH * IW), rem = v - zd * (IH * IW), zh = rem / IW, zw = rem - zh * IW;
        const int gd = od0 - 1 + zd, gh = zh - 1, gw = zw - 1;
        const bool ok = ((unsigned)gd < (unsigned)p.Di) & ((unsigned)gh < (unsigned)p.Hi) & ((unsigned)gw < (unsigned)p.Wi);
        offv[u] = idx < IELEM ? (ok ? __mul24(__mul24(gd, p.Hi) + gh, p.Wi) + gw : -1) : -2;
        ldso[u] = zd * PS + (zh * PW + zw) * 32 + ((cg ^ (zh & 1)) * 16);
    }
    const int wbase = cb0 * p.chunks * (KS * 64), wskip = (p.chunks - 1) * (KS * 64);
    f16x8 xr[PF], wr[WPF];
    float scu[16], shu[16];
    float slope_next = 1.f;
    auto issue = [&](int ch) {
        const int c_glob = ch * 16;
        const int s = (c_glob < p.src[0].C) ? 0 : 1;
        const int c_uni = c_glob - (s ? p.src[0].C : 0);
        const int sC = p.src[s].C;
        const int vs = FNN_VS(p.src[s]);                      // activation layout: fnn_device.h, SrcDesc
        const char *sp = (const char *)(p.src[s].ptr + (size_t)n * p.Di * p.Hi * p.Wi * sC + (c_uni >> 4) * FNN_CS(p.src[s]));
        slope_next = p.src[s].slope;
        const float *qs, *qh;
        fnn_ss_rows(p.src[s].ss, sC, n, c_uni, p.ident_ss, qs, qh);
#pragma unroll
        for (int j = 0; j < 16; ++j) { scu[j] = qs[j]; shu[j] = qh[j]; }
#pragma unroll
        for (int u = 0; u < PF; ++u)
            xr[u] = *(const f16x8 *)(sp + (unsigned)(((offv[u] >= 0 ? offv[u] : 0) * vs + cg * 8) * 2));
#pragma unroll
        for (int u = 0; u < WPF; ++u) {
            const int idx = tid + u * NT, idc = idx < WTOT ? idx : WTOT - 1;
            int e = idc + (idc >= KS * 64 ? wskip : 0);
            asm volatile("" : "+v"(e));                       // (a hoisted 64-bit address per element costs registers)
            wr[u] = *(const f16x8 *)((const char *)p.wpk + (unsigned)((wbase + e + ch * (KS * 64)) * 16));
        }
    };
    auto commit = [&]() {
        const f16 slope_h = (f16)slope_next;
        float sc[8], sh[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { sc[j] = cg ? scu[8 + j] : scu[j]; sh[j] = cg ? shu[8 + j] : shu[j]; }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            if ((u + 1) * NT > IELEM && offv[u] == -2) continue;
            f16x8 o = fnn_norm_leaky8(xr[u], sc, sh, slope_h);
            if (offv[u] < 0) o = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};      // the conv's zero padding
            *(f16x8 *)(sA + ldso[u]) = o;
        }
#pragma unroll
        for (int u = 0; u < WPF; ++u) {
            const int idx = tid + u * NT;
            if ((u + 1) * NT <= WTOT || idx < WTOT) ((f16x8 *)sW)[idx] = wr[u];
        }
    };
    int toff[5];
    f32x4 acc[TD][NB];
    auto kloop = [&]() { zr_kloop<TD, NB, KS>(acc, sA, toff, sW, lane, [](int pl) { return pl * PS; }); };

    issue(0);
    __builtin_amdgcn_sched_barrier(0);
    zr_tap_offsets<PW, true>(toff, lane, [=](int r) { return 4 * bh + (r >> 2); }, [=](int r) { return 4 * bw + (r & 3); });   // the wave's 4 x 4 block
#pragma unroll
    for (int j = 0; j < TD; ++j)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[j][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    commit();
    __syncthreads();
    for (int ch = 0; ch + 1 < p.chunks; ++ch) {
        issue(ch + 1);
        kloop();
        __syncthreads();
        commit();
        __syncthreads();
    }
    kloop();

    // ---- epilogue: bias, 16-byte stores (the interleaved cout order: lane quarter q holds channels q * 8 .. + 7), statistics
    {
        const int q = lane >> 4, r = lane & 15;
        float4 bv[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) bv[nb] = *(const float4 *)(p.bias + cb0 * 16 + q * 8 + nb * 4);
        float t1[NB][4], t2[NB][4];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int j = 0; j < 4; ++j) { t1[nb][j] = 0.f; t2[nb][j] = 0.f; }
        zr_epilogue_pair<TD>(p, acc, bv, n, od0, 4 * bh + (r >> 2), 4 * bw + (r & 3), cb0, lane, t1, t2);
        if (p.stats_out) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float a = row16_sum(t1[nb][j]), b = row16_sum(t2[nb][j]);
                    if (r == 0) {
                        const int c = q * 8 + nb * 4 + j;
                        sRed[(wave * 32 + c) * 2] = a;
                        sRed[(wave * 32 + c) * 2 + 1] = b;
                    }
                }
            __syncthreads();
            if (tid < 64) {
                const int c = tid >> 1, which = tid & 1;
                double v = 0;
#pragma unroll
                for (int w = 0; w < 9; ++w) v += (double)sRed[(w * 32 + c) * 2 + which];
                p.stats_out[(((size_t)n * p.stats_slots + td) * p.Cout + cb0 * 16 + c) * 2 + which] = v;
            }
        }
    }
}

template <int TD>
static int launch_zr12(ConvParams p, hipStream_t st) {
    p.tile_d = TD;
    p.tiles_d = (p.Do + TD - 1) / TD; p.tiles_h = 1; p.tiles_w = 1;
    p.ident_ss = conv3d_identity_ss();
    if (!p.ident_ss) return -2;
    dim3 grid(p.N * p.tiles_d, (p.Cout / 16) / 2);
    return fnn_launch_lds<conv3d_zr12_kernel<TD>>(grid, dim3(576), Zr12Lds<TD, 9>::bytes(), st, p);
}

// ----------------------------------------------------------------------------
// in-plane stride 2, depth stride 1 (the first down-sampling conv of an anisotropic network)
// ----------------------------------------------------------------------------
// The linear-tap persistent kernel serves this layer with 2 x 8 x 8 output tiles: four halo planes staged per two
// output planes (a timing-only build that staged half of them ran 21 % faster).  Here the depth-shift form: an
// 8 x 4 x 8 output tile, halo 10 x 9 x 17 voxels = 1.25 planes per output plane (and 30 % fewer staged voxels per
// output overall); wave = (pair of h rows, half of the depth slices): its operand of halo plane p for an in-plane tap
// pair serves the three depth taps of its output slices p, p - 1, p - 2 - 6 activation + 6 weight reads for 24 MFMAs.
// The operand's 8 voxels per row lie 64 bytes apart (2-way conflicted reads, like the linear-tap strided kernels; a
// de-interleaved image was slower there).  Same weight packing (FNN_PACK_ZR, interleaved cout order), statistics row per
// tile and epilogue as the stride-1 kernel.
template <int NB>
__global__ __launch_bounds__(256, 2) void conv3d_zs_kernel(const ConvParams p) {
    static_assert(NB == 2, "two cout blocks per workgroup");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    using L = ZsLds<NB, false>;
    constexpr int TD = 8, TH = 4, TDW = 4;                    // output tile depth x height (x 8 wide); depth slices per wave
    constexpr int ID = TD + 2, IH = 2 * TH + 1, IW = 17, PW = L::PW;
    constexpr int PS = L::PS, ABYTES = L::image;
    constexpr int KS = 15;
    constexpr int IELEM = ID * IH * IW * 2;
    constexpr int PF = (IELEM + 255) / 256;
    constexpr int WTOT = NB * KS * 64;
    constexpr int WPF = (WTOT + 255) / 256;

    int t = fnn_xcd_tile(gridDim.x, blockIdx.x);
    const int tw = t % p.tiles_w; t /= p.tiles_w;
    const int th = t % p.tiles_h; t /= p.tiles_h;
    const int td = t % p.tiles_d;
    const int n = t / p.tiles_d;
    const int cb0 = blockIdx.y * NB;
    const int od0 = td * TD, oh0 = th * TH, ow0 = tw * 8;
    const int hp = wave & 1, dh = wave >> 1;                  // this wave: output rows 2 hp, 2 hp + 1; depth slices 4 dh .. 4 dh + 3

    char *sA = smem;                                          // halo image: [ID][IH][PW] voxels x 32 B
    char *sW = smem + ABYTES;                                 // [NB][15][64 lanes][16 B]
    float *sBias = (float *)(sW + L::weights);

    int toff[5];
    f32x4 acc[TDW][NB];
    const int cg = tid & 1;
    int offv[PF], ldso[PF];
    {
        const int id0 = od0 - 1, ih0 = 2 * oh0 - 1, iw0 = 2 * ow0 - 1;
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int idx = tid + u * 256;
            const int v = idx >> 1;
            const int zd = v / (IH * IW), rem = v - zd * (IH * IW), zh = rem / IW, zw = rem - zh * IW;
            const int gd = id0 + zd, gh = ih0 + zh, gw = iw0 + zw;
            const bool ok = ((unsigned)gd < (unsigned)p.Di) & ((unsigned)gh < (unsigned)p.Hi) & ((unsigned)gw < (unsigned)p.Wi);
            const int lin = __mul24(__mul24(gd, p.Hi) + gh, p.Wi) + gw;
            offv[u] = idx < IELEM ? (ok ? lin : -1) : -2;
            ldso[u] = zd * PS + (zh * PW + zw) * 32 + cg * 16;
        }
    }
    int wofs[WPF];
#pragma unroll
    for (int u = 0; u < WPF; ++u) {
        const int idx = tid + u * 256;
        const int idc = idx < WTOT ? idx : WTOT - 1;
        const int nb = idc >= KS * 64 ? 1 : 0;
        wofs[u] = (cb0 + nb) * p.chunks * (KS * 64) + idc - nb * (KS * 64);
    }
    f16x8 xr[PF], wr[WPF];
    float scu[16], shu[16];
    float slope_next = 1.f;

    auto issue = [&](int ch) {
        const int c_glob = ch * 16;
        const int s = (c_glob < p.src[0].C) ? 0 : 1;
        const int c_uni = c_glob - (s ? p.src[0].C : 0);
        const int sC = p.src[s].C;
        const int vs = FNN_VS(p.src[s]);                      // activation layout: fnn_device.h, SrcDesc
        const char *sp = (const char *)(p.src[s].ptr + (size_t)n * p.Di * p.Hi * p.Wi * sC + (c_uni >> 4) * FNN_CS(p.src[s]));
        slope_next = p.src[s].slope;
        // (fnn_ss_rows' text, kept here: through the helper the kernel's SGPR spills moved, 10 -> 6)
        const float *qs = p.src[s].ss ? p.src[s].ss + (size_t)(2 * n) * sC + c_uni : p.ident_ss + c_uni;
        const float *qh = p.src[s].ss ? qs + sC : p.ident_ss + 512 + c_uni;
#pragma unroll
        for (int j = 0; j < 16; ++j) { scu[j] = qs[j]; shu[j] = qh[j]; }
#pragma unroll
        for (int u = 0; u < PF; ++u)
            xr[u] = *(const f16x8 *)(sp + (unsigned)(((offv[u] >= 0 ? offv[u] : 0) * vs + cg * 8) * 2));
#pragma unroll
        for (int u = 0; u < WPF; ++u) wr[u] = *(const f16x8 *)((const char *)p.wpk + (unsigned)((wofs[u] + ch * (KS * 64)) * 16));
    };
    auto commit = [&]() {
        const f16 slope_h = (f16)slope_next;
        float sc[8], sh[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { sc[j] = cg ? scu[8 + j] : scu[j]; sh[j] = cg ? shu[8 + j] : shu[j]; }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            if ((u + 1) * 256 > IELEM && offv[u] == -2) continue;
            f16x8 o = fnn_norm_leaky8(xr[u], sc, sh, slope_h);
            if (offv[u] < 0) o = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
            *(f16x8 *)(sA + ldso[u]) = o;
        }
#pragma unroll
        for (int u = 0; u < WPF; ++u) {
            const int idx = tid + u * 256;
            if ((u + 1) * 256 <= WTOT || idx < WTOT) ((f16x8 *)sW)[idx] = wr[u];
        }
    };
    auto kloop = [&]() { zr_kloop<TDW, NB, KS>(acc, sA, toff, sW, lane, [](int pl) { return pl * PS; }); };

    if (tid < NB * 16) sBias[tid] = p.bias[cb0 * 16 + tid];
    issue(0);
    __builtin_amdgcn_sched_barrier(0);
    // the wave's two output rows from its first plane on; the voxel's input position is twice its output position + the tap
    zr_tap_offsets<PW, false>(toff, lane, [=](int r) { return 2 * (2 * hp + (r >> 3)); }, [](int r) { return 2 * (r & 7); }, (TDW * dh) * PS);
#pragma unroll
    for (int j = 0; j < TDW; ++j)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[j][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};

    commit();
    __syncthreads();
    for (int ch = 0; ch + 1 < p.chunks; ++ch) {
        issue(ch + 1);
        kloop();
        __syncthreads();
        commit();
        __syncthreads();
    }
    kloop();
    __syncthreads();

    // ---- epilogue: bias, fp16 store (16 bytes per lane: the interleaved cout order), statistics
    {
        const int q = lane >> 4, r = lane & 15;
        float4 bv[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) bv[nb] = *(const float4 *)(sBias + q * 8 + nb * 4);
        float t1[NB][4], t2[NB][4];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int j = 0; j < 4; ++j) { t1[nb][j] = 0.f; t2[nb][j] = 0.f; }
        zr_epilogue_pair<TDW>(p, acc, bv, n, od0 + TDW * dh, oh0 + 2 * hp + (r >> 3), ow0 + (r & 7), cb0, lane, t1, t2);
        if (p.stats_out) stats_to_global<NB, true, true>(p, t1, t2, (float *)smem, n, cb0, wave, lane, tid, (td * p.tiles_h + th) * p.tiles_w + tw);
    }
}

// Persistent form of conv3d_zs_kernel for single-chunk layers (Cin <= 16: the first down-sampling conv).  With one
// chunk a tile is ONE k-loop of 120 MFMAs per wave behind a serial chain - table set-up, the halo's round trip, its
// normalisation into LDS, then the epilogue - and two workgroups per CU cannot cover that chain for each other: the
// layer ran at a workgroup lifetime of ~8 us per tile.  Here a workgroup walks tiles (those of its XCD interleaved
// with the other workgroups', so that the tiles in flight on an XCD stay neighbours in L2): the 30 KB of weight
// fragments are loaded once, the per-thread LDS offsets are computed once, and the next tile's halo loads are in
// flight during the k-loop and the epilogue of the current one.  Same tile, image, arithmetic and statistics row per
// tile as conv3d_zs_kernel: bit-identical results.
__global__ __launch_bounds__(256, 2) void conv3d_zsp_kernel(const ConvParams p, const int total_tiles) {
    constexpr int NB = 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    using L = ZsLds<NB, true>;
    constexpr int TD = 8, TH = 4, TDW = 4;
    constexpr int ID = TD + 2, IH = 2 * TH + 1, IW = 17, PW = L::PW;
    constexpr int PS = L::PS, ABYTES = L::image;
    constexpr int KS = 15;
    constexpr int IELEM = ID * IH * IW * 2;
    constexpr int PF = (IELEM + 255) / 256;
    constexpr int WTOT = NB * KS * 64;
    const int hp = wave & 1, dh = wave >> 1;

    char *sA = smem;
    char *sW = smem + ABYTES;                                 // [NB][15][64 lanes][16 B]: resident
    float *sRed = (float *)(sW + L::weights);                 // [4 waves][32][2]

    // this workgroup's tiles: t = first + i * stride inside its XCD's contiguous range
    int t_first, t_stride, t_end;
    {
        const int nwg = gridDim.x, idx = blockIdx.x >> 3;
        int wg_lo, wg_n;                                      // the XCD's workgroups
        fnn_xcd_range(nwg, blockIdx.x, wg_lo, wg_n);
        const int r_lo = (int)((long long)total_tiles * wg_lo / nwg), r_hi = (int)((long long)total_tiles * (wg_lo + wg_n) / nwg);
        t_first = r_lo + idx; t_stride = wg_n; t_end = r_hi;
    }
    if (t_first >= t_end) return;
    const int cb0 = blockIdx.y * NB;

    // ---- one-time set-up: weights, LDS offsets, operand offsets
    for (int idx = tid; idx < WTOT; idx += 256) {
        const int nb = idx >= KS * 64 ? 1 : 0;
        ((f16x8 *)sW)[idx] = ((const f16x8 *)p.wpk)[(cb0 + nb) * p.chunks * (KS * 64) + idx - nb * (KS * 64)];
    }
    const int cg = tid & 1;
    unsigned relp[PF / 2];                                    // halo coordinates, two 13-bit triples (zd : 4, zh : 4, zw : 5) per register
    static_assert(PF % 2 == 0, "pairs");
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const int idx = tid + u * 256, v = (idx < IELEM ? idx : IELEM - 1) >> 1;
        const int zd = v / (IH * IW), rem = v - zd * (IH * IW), zh = rem / IW, zw = rem - zh * IW;
        const unsigned t = (unsigned)((zd << 9) | (zh << 5) | zw);
        if (u & 1) relp[u >> 1] |= t << 16; else relp[u >> 1] = t;
    }
    const bool has_last = tid + (PF - 1) * 256 < IELEM;
#define ZSP_REL(u) ((relp[(u) >> 1] >> (((u) & 1) * 16)) & 0x1fffu)
    int toff[5];
    zr_tap_offsets<PW, false>(toff, lane, [=](int r) { return 2 * (2 * hp + (r >> 3)); }, [](int r) { return 2 * (r & 7); }, (TDW * dh) * PS);
    const int q = lane >> 4, r = lane & 15;
    float4 bv[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) bv[nb] = *(const float4 *)(p.bias + cb0 * 16 + q * 8 + nb * 4);

    int offv[PF];
    f16x8 xr[PF];
    float scu[16], shu[16];
    auto tile_coords = [&](int t, int &n, int &od0, int &oh0, int &ow0, int &slot) {
        const int tw = t % p.tiles_w; t /= p.tiles_w;
        const int th = t % p.tiles_h; t /= p.tiles_h;
        const int td = t % p.tiles_d;
        n = t / p.tiles_d;
        od0 = td * TD; oh0 = th * TH; ow0 = tw * 8;
        slot = (td * p.tiles_h + th) * p.tiles_w + tw;
    };
    auto set_offsets = [&](int od0, int oh0, int ow0) {
        const int id0 = od0 - 1, ih0 = 2 * oh0 - 1, iw0 = 2 * ow0 - 1;
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            unsigned t = ZSP_REL(u);
            asm volatile("" : "+v"(t));                       // keep the unpacked coordinates out of loop-invariant registers
            const unsigned gd = (unsigned)(id0 + (int)(t >> 9)), gh = (unsigned)(ih0 + (int)((t >> 5) & 15)), gw = (unsigned)(iw0 + (int)(t & 31));
            const bool ok = gd < (unsigned)p.Di && gh < (unsigned)p.Hi && gw < (unsigned)p.Wi;
            offv[u] = ok ? (int)(__umul24(__umul24(gd, (unsigned)p.Hi) + gh, (unsigned)p.Wi) + gw) : -1;
        }
    };
    auto issue = [&](int n) {
        const int sC = p.src[0].C;
        const int vs = FNN_VS(p.src[0]);
        const char *sp = (const char *)(p.src[0].ptr + (size_t)n * p.Di * p.Hi * p.Wi * sC);
        const float *qs, *qh;
        fnn_ss_rows(p.src[0].ss, sC, n, 0, p.ident_ss, qs, qh);
#pragma unroll
        for (int j = 0; j < 16; ++j) { scu[j] = qs[j]; shu[j] = qh[j]; }
#pragma unroll
        for (int u = 0; u < PF; ++u)
            xr[u] = *(const f16x8 *)(sp + (unsigned)(((offv[u] >= 0 ? offv[u] : 0) * vs + cg * 8) * 2));
    };
    auto commit = [&]() {
        const f16 slope_h = (f16)p.src[0].slope;
        float sc[8], sh[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { sc[j] = cg ? scu[8 + j] : scu[j]; sh[j] = cg ? shu[8 + j] : shu[j]; }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            f16x8 o = fnn_norm_leaky8(xr[u], sc, sh, slope_h);
            if (offv[u] < 0) o = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
            unsigned t = ZSP_REL(u);
            asm volatile("" : "+v"(t));
            const int zd = (int)(t >> 9), zh = (int)((t >> 5) & 15), zw = (int)(t & 31);
            if (u + 1 < PF || has_last) *(f16x8 *)(sA + zd * PS + (zh * PW + zw) * 32 + cg * 16) = o;
        }
    };

    int n_cur, od0, oh0, ow0, slot;
    tile_coords(t_first, n_cur, od0, oh0, ow0, slot);
    set_offsets(od0, oh0, ow0);
    issue(n_cur);
    commit();
    __syncthreads();                                          // weights + first image
    const f16x2 ones = {(f16)1.f, (f16)1.f};
    for (int t = t_first; t < t_end; t += t_stride) {
        // prefetch the next tile (the last one prefetches itself again: issue / commit stay unconditional)
        int n_nx = n_cur, d_nx = od0, h_nx = oh0, w_nx = ow0, s_nx = slot;
        if (t + t_stride < t_end) tile_coords(t + t_stride, n_nx, d_nx, h_nx, w_nx, s_nx);
        set_offsets(d_nx, h_nx, w_nx);
        issue(n_nx);
        f32x4 acc[TDW][NB];
#pragma unroll
        for (int j = 0; j < TDW; ++j)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[j][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int pr = 0; pr < 5; ++pr) {
            const char *bp = sA + toff[pr];
            f16x8 xf[TDW + 2];
#pragma unroll
            for (int pl = 0; pl < TDW + 2; ++pl) xf[pl] = *(const f16x8 *)(bp + pl * PS);
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
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- epilogue of tile t (as conv3d_zs_kernel): bias, 16-byte stores, statistics row.  (zr_kloop's text above and
        // zr_epilogue_pair's below, kept here: through either helper this kernel's register counts moved, 92 -> 94 SGPRs,
        // 208 -> 206 VGPRs)
        float t1[NB][4], t2[NB][4];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int j = 0; j < 4; ++j) { t1[nb][j] = 0.f; t2[nb][j] = 0.f; }
        {
            const unsigned item_bytes = (unsigned)p.Do * p.Ho * p.Wo * p.Cout * 2;
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(p.out + (size_t)n_cur * (item_bytes >> 1), 0, item_bytes, 0x00020000);
            const unsigned ovs2 = (unsigned)FNN_OVS(p) * 2;
            const unsigned coff = (unsigned)(cb0 + (q >> 1)) * (unsigned)(FNN_OCS(p) * 2) + (unsigned)(q & 1) * 16;   // output layout: fnn_device.h
            const int oh = oh0 + 2 * hp + (r >> 3), ow = ow0 + (r & 7);
            const bool ok_hw = oh < p.Ho && ow < p.Wo;
#pragma unroll
            for (int mb = 0; mb < TDW; mb += 2) {
                f16x8 o[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int od = od0 + TDW * dh + mb + h;
                    const bool ok = ok_hw && od < p.Do;
                    const unsigned voff = ok ? (unsigned)((od * p.Ho + oh) * p.Wo + ow) * ovs2 + coff : 0x80000000u;
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) {
                        o[h][nb * 4 + 0] = (f16)(acc[mb + h][nb][0] + bv[nb].x);
                        o[h][nb * 4 + 1] = (f16)(acc[mb + h][nb][1] + bv[nb].y);
                        o[h][nb * 4 + 2] = (f16)(acc[mb + h][nb][2] + bv[nb].z);
                        o[h][nb * 4 + 3] = (f16)(acc[mb + h][nb][3] + bv[nb].w);
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
        if (p.stats_out) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float a = row16_sum(t1[nb][j]), b = row16_sum(t2[nb][j]);
                    if (r == 0) {
                        const int c = q * 8 + nb * 4 + j;              // the interleaved cout order (conv3d_pack_cout)
                        sRed[(wave * 32 + c) * 2] = a;
                        sRed[(wave * 32 + c) * 2 + 1] = b;
                    }
                }
        }
        __syncthreads();                                      // every wave is done reading the image; sRed complete
        if (p.stats_out && tid < 64) {
            const int c = tid >> 1, which = tid & 1;
            double v = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) v += (double)sRed[(w * 32 + c) * 2 + which];
            p.stats_out[(((size_t)n_cur * p.stats_slots + slot) * p.Cout + cb0 * 16 + c) * 2 + which] = v;
        }
        commit();
        __syncthreads();
        n_cur = n_nx; od0 = d_nx; oh0 = h_nx; ow0 = w_nx; slot = s_nx;
    }
#undef ZSP_REL
}

// The single-chunk strided layer WALKING along d (round 4; conv3d_zrw_kernel's walk with conv3d_zs_kernel's tile).
// conv3d_zsp_kernel re-staged its whole 10 x 9 x 17 halo for every 8 x 4 x 8 tile: 1.49 input voxels read per input voxel
// of the layer.  A workgroup here owns one 4 x 8 in-plane window (9 x 17 input columns) and walks `tps` consecutive
// d-tiles: the image is a RING of ten planes - a tile brings eight new ones (1.20 voxels per voxel), the next tile's
// planes are in flight during the k-loop - the weights are staged once, and the staging is the column walk of the ZR
// kernels: a thread owns one (row, column, channel half) of the window (306 of them: threads 0 .. 49 own a second one),
// its address is one constant + a scalar per plane, columns outside the tensor read zeros through the buffer's range
// check.  Same image layout, operand offsets, k-loop, epilogue and statistics row per tile as conv3d_zsp_kernel:
// bit-identical results.
__global__ __launch_bounds__(256, 2) void conv3d_zsw_kernel(const ConvParams p, const int segs, const int tps) {
    constexpr int NB = 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    using L = ZsLds<NB, true>;
    constexpr int TD = 8, TH = 4, TDW = 4;
    constexpr int ID = TD + 2, IH = 2 * TH + 1, IW = 17, PW = L::PW;
    constexpr int PS = L::PS, ABYTES = L::image;
    constexpr int KS = 15, WB = KS * 64, WPB = (WB + 255) / 256;
    constexpr int NCOL = IH * IW * 2;                         // 306 (row, column, half) elements per plane
    const int hp = wave & 1, dh = wave >> 1;

    int t = __builtin_amdgcn_readfirstlane(fnn_xcd_tile(gridDim.x, blockIdx.x));
    const int tw = __builtin_amdgcn_readfirstlane(t % p.tiles_w); t = __builtin_amdgcn_readfirstlane(t / p.tiles_w);
    const int th = __builtin_amdgcn_readfirstlane(t % p.tiles_h); t = __builtin_amdgcn_readfirstlane(t / p.tiles_h);
    const int seg = __builtin_amdgcn_readfirstlane(t % segs);
    const int n = __builtin_amdgcn_readfirstlane(t / segs);
    const int td0 = seg * tps, td1 = td0 + tps < p.tiles_d ? td0 + tps : p.tiles_d;
    if (td0 >= td1) return;
    const int cb0 = blockIdx.y * NB;
    const int oh0 = th * TH, ow0 = tw * 8;

    char *sA = smem;                                          // ring of ID halo planes: plane 8 td0 - 1 + k sits in slot k % ID
    char *sW = smem + ABYTES;                                 // [NB][15][64 lanes][16 B], resident
    float *sRed = (float *)(sW + L::weights);                 // [4 waves][32][2]

    // ---- this thread's one or two elements of a plane
    const int sC = p.src[0].C, vs = FNN_VS(p.src[0]);
    const unsigned item_bytes = (unsigned)p.Di * p.Hi * p.Wi * sC * 2;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void *)(p.src[0].ptr + (size_t)n * (item_bytes >> 1)), 0, item_bytes, 0x00020000);
    const unsigned plane_bytes = (unsigned)p.Hi * p.Wi * vs * 2;
    const int cg = tid & 1;
    unsigned voff[2];
    int ldso[2];
    bool has[2], okc[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = tid + 256 * k;
        has[k] = e < NCOL;
        const int col = (has[k] ? e : 0) >> 1;
        const int zh = (col * 241) >> 12, zw = col - zh * IW;   // col / 17 for col < 153
        const int gh = 2 * oh0 - 1 + zh, gw = 2 * ow0 - 1 + zw;
        okc[k] = has[k] & ((unsigned)gh < (unsigned)p.Hi) & ((unsigned)gw < (unsigned)p.Wi);
        voff[k] = okc[k] ? (unsigned)(__mul24(gh, p.Wi) + gw) * (unsigned)(vs * 2) + cg * 16 : 0x80000000u;
        ldso[k] = (zh * PW + zw) * 32 + cg * 16;
    }
    const f16 slope_h = (f16)p.src[0].slope;
    // conv3d_zsp_kernel's arithmetic: the fp32 rows, rounded to fp16 by fnn_norm8 (stats_finalize_kernel's ssh rows hold the same roundings)
    float sc[8], sh[8];
    {
        const float *qs, *qh;
        fnn_ss_rows(p.src[0].ss, sC, n, 0, p.ident_ss, qs, qh);
#pragma unroll
        for (int j = 0; j < 8; ++j) { sc[j] = qs[cg * 8 + j]; sh[j] = qh[cg * 8 + j]; }
    }

    fnn_u32x4v xr[2][ID];
    auto load_planes = [&](int td, int u0) {                  // the planes u0 .. 9 of tile td: 8 td - 1 + u, clamped (see stage())
#pragma unroll
        for (int u = 0; u < ID; ++u) {
            if (u < u0) continue;
            int gd = td * TD - 1 + u;
            gd = gd < 0 ? 0 : (gd >= p.Di ? p.Di - 1 : gd);
#pragma unroll
            for (int k = 0; k < 2; ++k)
                xr[k][u] = __builtin_bit_cast(fnn_u32x4v, __builtin_amdgcn_raw_buffer_load_b128(rx, voff[k], (unsigned)gd * plane_bytes, 0));
        }
    };
    auto stage = [&](int td, int u0) {                        // normalise + LeakyReLU, into the planes' ring slots; outside the tensor: zeros
        const int k0 = (td - td0) * TD;
#pragma unroll
        for (int u = 0; u < ID; ++u) {
            if (u < u0) continue;
            const int gd = td * TD - 1 + u;                   // (scalar)
            const bool plane_ok = (unsigned)gd < (unsigned)p.Di;
            char *dst = sA + ((k0 + u) % ID) * PS;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                f16x8 o = fnn_norm_leaky8(__builtin_bit_cast(f16x8, xr[k][u]), sc, sh, slope_h);
                if (!okc[k] || !plane_ok) o = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};     // the conv's zero padding
                if (has[k]) *(f16x8 *)(dst + ldso[k]) = o;
            }
        }
    };
    int toff[5];
    zr_tap_offsets<PW, false>(toff, lane, [=](int r) { return 2 * (2 * hp + (r >> 3)); }, [](int r) { return 2 * (r & 7); });
    const int q = lane >> 4, r = lane & 15;
    float4 bv[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) bv[nb] = *(const float4 *)(p.bias + cb0 * 16 + q * 8 + nb * 4);
    f32x4 acc[TDW][NB];
    auto kloop = [&](int td) {
        const int k0 = (td - td0) * TD + TDW * dh;            // the wave's first plane of the tile's ten
        int roff[TDW + 2];                                    // (scalars) where its six planes sit in the ring
#pragma unroll
        for (int pl = 0; pl < TDW + 2; ++pl) roff[pl] = ((k0 + pl) % ID) * PS;
#pragma unroll
        for (int j = 0; j < TDW; ++j)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[j][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
        zr_kloop<TDW, NB, KS>(acc, sA, toff, sW, lane, [&](int pl) { return roff[pl]; });
    };
    auto finish = [&](int td) {                               // conv3d_zsp_kernel's epilogue: bias, 16-byte stores, statistics row (+ a barrier)
        const int od0 = td * TD;
        float t1[NB][4], t2[NB][4];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int j = 0; j < 4; ++j) { t1[nb][j] = 0.f; t2[nb][j] = 0.f; }
        zr_epilogue_pair<TDW>(p, acc, bv, n, od0 + TDW * dh, oh0 + 2 * hp + (r >> 3), ow0 + (r & 7), cb0, lane, t1, t2);
        if (p.stats_out) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float a = row16_sum(t1[nb][j]), b = row16_sum(t2[nb][j]);
                    if (r == 0) {
                        const int c = q * 8 + nb * 4 + j;              // the interleaved cout order (conv3d_pack_cout)
                        sRed[(wave * 32 + c) * 2] = a;
                        sRed[(wave * 32 + c) * 2 + 1] = b;
                    }
                }
        }
        __syncthreads();                                      // sRed complete (and the planes staged before this call are published)
        if (p.stats_out && tid < 64) {
            const int c = tid >> 1, which = tid & 1;
            double v = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) v += (double)sRed[(w * 32 + c) * 2 + which];
            p.stats_out[(((size_t)n * p.stats_slots + (td * p.tiles_h + th) * p.tiles_w + tw) * p.Cout + cb0 * 16 + c) * 2 + which] = v;
        }
    };

    // ---- prologue: the first tile's ten planes and the weights
    load_planes(td0, 0);
    fnn_u32x4v wr[NB][WPB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const f16 *wp = p.wpk + ((size_t)((cb0 + nb) * p.chunks) * WB) * 8;
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void *)wp, 0, WB * 16, 0x00020000);
#pragma unroll
        for (int u = 0; u < WPB; ++u) wr[nb][u] = __builtin_bit_cast(fnn_u32x4v, __builtin_amdgcn_raw_buffer_load_b128(rw, tid * 16, u * 4096, 0));
    }
    stage(td0, 0);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int u = 0; u < WPB; ++u)
            if (u + 1 < WPB || wave < 3) *(fnn_u32x4v *)(sW + ((nb * WB + u * 256) + tid) * 16) = wr[nb][u];
    __syncthreads();

    // ---- the walk: the last tile is peeled off (nothing to prefetch behind it)
    for (int td = td0; td + 1 < td1; ++td) {
        load_planes(td + 1, 2);                               // eight new planes, in flight during the MFMAs
        kloop(td);
        __syncthreads();                                      // every wave is done with this tile's planes (and with sRed of the previous tile)
        stage(td + 1, 2);                                     // over the slots of this tile's first eight planes
        finish(td);                                           // (its barrier also publishes the staged planes)
    }
    kloop(td1 - 1);
    __syncthreads();
    finish(td1 - 1);
}

static int launch_zs(ConvParams p, const ConvChoice &c, hipStream_t st) {
    p.tile_d = 8;
    p.tiles_d = (p.Do + 7) / 8;
    p.tiles_h = (p.Ho + 3) / 4;
    p.tiles_w = (p.Wo + 7) / 8;
    fnn_allow_lds<conv3d_zs_kernel<2>>();
    p.ident_ss = conv3d_identity_ss();
    if (!p.ident_ss) return -2;
    const int total = p.N * p.tiles_d * p.tiles_h * p.tiles_w, groups = (p.Cout / 16) / 2;
    if (c.kernel == CK_ZSW) {
        return fnn_launch_lds<conv3d_zsw_kernel>(dim3(p.N * p.tiles_h * p.tiles_w * c.segs, groups), dim3(256), ZsLds<2, true>::bytes(), st, p, c.segs, c.tps);
    }
    if (c.kernel == CK_ZSP) {
        return fnn_launch_lds<conv3d_zsp_kernel>(dim3(c.gx, groups), dim3(256), ZsLds<2, true>::bytes(), st, p, total);
    }
    return fnn_launch_lds<conv3d_zs_kernel<2>>(dim3(total, groups), dim3(256), ZsLds<2, false>::bytes(), st, p);
}

// ----------------------------------------------------------------------------
// fp8 (OCP e4m3) variant: BASELINE config 5's "fp8 MFMA conv path"
// ----------------------------------------------------------------------------
// Same tiling, staging and depth-shift reuse; what changes is the operand format of the matrix cores:
//   activations  the normalised + LeakyReLU'd value times p.act_mult (8: unit-variance data sits at 2^3, e4m3 reaches
//                448 = 56 sigma; below 2^-9 * 8 it flushes) is converted with v_cvt_pk_fp8_f32 (round to nearest even,
//                clamped to +-448) while it is staged: 8 B per (voxel, 8 channels) in LDS instead of 16;
//   weights      e4m3 on the host with one scale per output channel (max |w| -> 448), packed in the same fragment
//                order at 8 B per lane;
//   MFMA         v_mfma_f32_16x16x32_fp8_fp8, fp32 accumulation; the epilogue multiplies by w_scale[cout] / act_mult
//                (p.oscale) before the bias, the fp16 store and the statistics, which stay as in the fp16 kernel.
// The non-scaled fp8 MFMA issues at the f16 rate on gfx950 (MI355X_MICROARCH.md, Matrix cores): this path halves the
// LDS and weight traffic, not the matrix time; the 2x rate needs the MX-scaled K = 128 form.
// LDS image: [plane][row][8-channel half][24 slots of 8 B] - sub-row pitch 192 B puts the four 64-byte segments a
// 32-lane ds_read_b64 group touches (2 rows x 2 halves) into four different bank quarters: conflict free.
typedef long fnn_i64;
typedef unsigned fnn_u32x4 __attribute__((ext_vector_type(4)));      // (HIP's uint4 struct arrays go to scratch)
template <int NB, int TD>
__global__ __launch_bounds__(256, 2) void conv3d_zr8_kernel(const ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    using L = Zr8Lds<NB, TD>;
    constexpr int IH = 10, IW = 10, ID = TD + 2;
    constexpr int SUB = L::SUB, PS = L::PS, ABYTES = L::image;   // sub-row pitch, bytes per halo plane
    constexpr int KS = 15;
    constexpr int IELEM = ID * IH * IW * 2;
    constexpr int PF = (IELEM + 255) / 256;
    constexpr int WTOT = NB * KS * 32;                        // 16-byte pieces (two lanes' fragments) per chunk
    constexpr int WPF = (WTOT + 255) / 256;

    int t = fnn_xcd_tile(gridDim.x, blockIdx.x);
    const int tw = t % p.tiles_w; t /= p.tiles_w;
    const int th = t % p.tiles_h; t /= p.tiles_h;
    const int td = t % p.tiles_d;
    const int n = t / p.tiles_d;
    const int cb0 = blockIdx.y * NB;
    const int od0 = td * TD, oh0 = th * 8, ow0 = tw * 8;

    char *sA = smem;
    char *sW = smem + ABYTES;                                 // [NB][15][64 lanes][8 B]
    float *sBias = (float *)(sW + L::weights);                // [NB * 16] bias, then [NB * 16] output scales

    int toff[5];
    f32x4 acc[TD][NB];
    const int cg = tid & 1;
    int offv[PF], ldso[PF];
    {
        const int id0 = od0 - 1, ih0 = oh0 - 1, iw0 = ow0 - 1;
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int idx = tid + u * 256;
            const int v = idx >> 1;
            const int zd = v / (IH * IW), rem = v - zd * (IH * IW), zh = rem / IW, zw = rem - zh * IW;
            const int gd = id0 + zd, gh = ih0 + zh, gw = iw0 + zw;
            const bool ok = gd >= 0 && gd < p.Di && gh >= 0 && gh < p.Hi && gw >= 0 && gw < p.Wi;
            offv[u] = idx < IELEM ? (ok ? (gd * p.Hi + gh) * p.Wi + gw : -1) : -2;
            ldso[u] = zd * PS + (zh * 2 + cg) * SUB + zw * 8;
        }
    }
    int wofs[WPF];
#pragma unroll
    for (int u = 0; u < WPF; ++u) {
        const int idx = tid + u * 256;
        const int idc = idx < WTOT ? idx : WTOT - 1;
        const int nb = idc >= KS * 32 ? 1 : 0;                // NB <= 2
        wofs[u] = (cb0 + nb) * p.chunks * (KS * 32) + idc - nb * (KS * 32);
    }
    f16x8 xr[PF];
    fnn_u32x4 wr[WPF];
    float4 scr[2], shr[2];
    float slope_next = 1.f;

    auto issue = [&](int ch) {
        const int c_glob = ch * 16;
        const int s = (c_glob < p.src[0].C) ? 0 : 1;
        const int c_uni = c_glob - (s ? p.src[0].C : 0);
        const int c_loc = c_uni + cg * 8;
        const int sC = p.src[s].C;
        const int vs = FNN_VS(p.src[s]);                      // activation layout: fnn_device.h, SrcDesc
        const char *sp = (const char *)(p.src[s].ptr + (size_t)n * p.Di * p.Hi * p.Wi * sC + (c_uni >> 4) * FNN_CS(p.src[s]));
        slope_next = p.src[s].slope;
        // (fnn_ss_rows' text, kept here: through the helper every instantiation took three more SGPRs)
        const float *qs = p.src[s].ss ? p.src[s].ss + (size_t)(2 * n) * sC + c_loc : p.ident_ss + c_loc;
        const float *qh = p.src[s].ss ? qs + sC : p.ident_ss + 512 + c_loc;
        scr[0] = *(const float4 *)qs; scr[1] = *(const float4 *)(qs + 4);
        shr[0] = *(const float4 *)qh; shr[1] = *(const float4 *)(qh + 4);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < PF; ++u)
            xr[u] = *(const f16x8 *)(sp + (unsigned)(((offv[u] >= 0 ? offv[u] : 0) * vs + cg * 8) * 2));
#pragma unroll
        for (int u = 0; u < WPF; ++u) wr[u] = *(const fnn_u32x4 *)((const char *)p.wpk + (unsigned)((wofs[u] + ch * (KS * 32)) * 16));
    };
    auto commit = [&]() {
        const float am = p.act_mult, slope = slope_next;
        // LeakyReLU commutes with a positive factor: the fp8 multiplier goes into scale and shift
        const float sc[8] = {scr[0].x * am, scr[0].y * am, scr[0].z * am, scr[0].w * am, scr[1].x * am, scr[1].y * am, scr[1].z * am, scr[1].w * am};
        const float sh[8] = {shr[0].x * am, shr[0].y * am, shr[0].z * am, shr[0].w * am, shr[1].x * am, shr[1].y * am, shr[1].z * am, shr[1].w * am};
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            if ((u + 1) * 256 > IELEM && offv[u] == -2) continue;
            auto q = [&](int j) {
                const float v = fmaf((float)xr[u][j], sc[j], sh[j]);
                return __builtin_amdgcn_fmed3f(fmaxf(v, v * slope), -448.f, 448.f);
            };
            int lo = 0, hi = 0;
            lo = __builtin_amdgcn_cvt_pk_fp8_f32(q(0), q(1), lo, false);
            lo = __builtin_amdgcn_cvt_pk_fp8_f32(q(2), q(3), lo, true);
            hi = __builtin_amdgcn_cvt_pk_fp8_f32(q(4), q(5), hi, false);
            hi = __builtin_amdgcn_cvt_pk_fp8_f32(q(6), q(7), hi, true);
            if (offv[u] < 0) { lo = 0; hi = 0; }               // the conv's zero padding
            *(int2 *)(sA + ldso[u]) = make_int2(lo, hi);
        }
#pragma unroll
        for (int u = 0; u < WPF; ++u) {
            const int idx = tid + u * 256;
            if ((u + 1) * 256 <= WTOT || idx < WTOT) ((fnn_u32x4 *)sW)[idx] = wr[u];
        }
    };
    auto kloop = [&]() {
#pragma unroll
        for (int pr = 0; pr < 5; ++pr) {
            const char *bp = sA + toff[pr];
            fnn_i64 xf[ID];
#pragma unroll
            for (int pl = 0; pl < ID; ++pl) xf[pl] = *(const fnn_i64 *)(bp + pl * PS);
#pragma unroll
            for (int dz = 0; dz < 3; ++dz) {
                fnn_i64 wf[NB];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) wf[nb] = *(const fnn_i64 *)(sW + ((nb * KS + pr * 3 + dz) * 64 + lane) * 8);
#pragma unroll
                for (int j = 0; j < TD; ++j)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
                        acc[j][nb] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wf[nb], xf[j + dz], acc[j][nb], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    issue(0);
    __builtin_amdgcn_sched_barrier(0);
    if (tid < NB * 16) { sBias[tid] = p.bias[cb0 * 16 + tid]; sBias[NB * 16 + tid] = p.oscale[cb0 * 16 + tid]; }
    zr_tap_offsets(toff, lane, [=](int r) { return 2 * wave + (r >> 3); }, [](int r) { return r & 7; }, [](int row, int col, int kh) { return (row * 2 + kh) * SUB + col * 8; });
#pragma unroll
    for (int j = 0; j < TD; ++j)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[j][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};

    commit();
    __syncthreads();
    for (int ch = 0; ch + 1 < p.chunks; ++ch) {
        issue(ch + 1);
        kloop();
        __syncthreads();
        commit();
        __syncthreads();
    }
    kloop();
    __syncthreads();
    {
        float4 bv[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int co = NB == 2 ? (lane >> 4) * 8 + nb * 4 : nb * 16 + (lane >> 4) * 4;
            bv[nb] = *(const float4 *)(sBias + co);
            const float4 sv = *(const float4 *)(sBias + NB * 16 + co);
#pragma unroll
            for (int j = 0; j < TD; ++j) {
                acc[j][nb][0] *= sv.x; acc[j][nb][1] *= sv.y; acc[j][nb][2] *= sv.z; acc[j][nb][3] *= sv.w;
            }
        }
        float t1[NB][4], t2[NB][4];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int j = 0; j < 4; ++j) { t1[nb][j] = 0.f; t2[nb][j] = 0.f; }
        if constexpr (NB == 2) zr_epilogue_pair<TD>(p, acc, bv, n, od0, oh0 + 2 * wave + ((lane & 15) >> 3), ow0 + (lane & 7), cb0, lane, t1, t2);
        else tile_epilogue<NB, TD, true>(p, acc, bv, n, od0, oh0, ow0, cb0, wave, lane, t1, t2);
        if (p.stats_out) stats_to_global<NB, true, NB == 2>(p, t1, t2, (float *)smem, n, cb0, wave, lane, tid, (td * p.tiles_h + th) * p.tiles_w + tw);
    }
}

template <int NB, int TD>
static int launch_zr8(ConvParams p, hipStream_t st) {
    p.tile_d = TD;
    p.tiles_d = (p.Do + TD - 1) / TD;
    p.tiles_h = (p.Ho + 7) / 8;
    p.tiles_w = (p.Wo + 7) / 8;
    p.ident_ss = conv3d_identity_ss();
    if (!p.ident_ss || !p.oscale) return -2;
    dim3 grid(p.N * p.tiles_d * p.tiles_h * p.tiles_w, (p.Cout / 16) / NB);
    return fnn_launch_lds<conv3d_zr8_kernel<NB, TD>>(grid, dim3(256), Zr8Lds<NB, TD>::bytes(), st, p);
}

template <int NB, int TD, int TH = 8>
static int launch_zr(ConvParams p, hipStream_t st) {
    p.tile_d = TD;
    p.tiles_d = (p.Do + TD - 1) / TD;
    p.tiles_h = (p.Ho + 7) / 8;
    p.tiles_w = (p.Wo + 7) / 8;
    size_t lds = ZrLds<NB, TD, TH>::bytes();
    if (const char *pad = fnn_knob("FNN_ZR_LDS_PAD")) lds += (size_t)atoi(pad);      // A-B aid: fewer ZR workgroups per CU (room for another stream's kernels)
    p.ident_ss = conv3d_identity_ss();
    p.ident_ssh = conv3d_identity_ssh();
    if (!p.ident_ss || !p.ident_ssh) return -2;
    dim3 grid(p.N * p.tiles_d * p.tiles_h * p.tiles_w, (p.Cout / 16) / NB);
#ifdef FNN_TMODE
    p.tmode = getenv("FNN_ZR_TMODE") ? atoi(getenv("FNN_ZR_TMODE")) : 0;     // timing-only proxies (wrong results): tools/zr_tmode.py
#endif
    return fnn_launch_lds<conv3d_zr_kernel<NB, TD, TH>>(grid, dim3(TH * 32), lds, st, p);
}

// the walking form for single-chunk layers: `segs` d-segments of `tps` tiles per in-plane window
template <int NB>
static int launch_zrw(ConvParams p, const ConvChoice &c, hipStream_t st) {
    constexpr int TD = 8;
    p.tile_d = TD;
    p.tiles_d = (p.Do + TD - 1) / TD;
    p.tiles_h = (p.Ho + 7) / 8;
    p.tiles_w = (p.Wo + 7) / 8;
    p.ident_ss = conv3d_identity_ss();
    p.ident_ssh = conv3d_identity_ssh();
    if (!p.ident_ss || !p.ident_ssh) return -2;
    dim3 grid(p.N * p.tiles_h * p.tiles_w * c.segs, (p.Cout / 16) / NB);
    return fnn_launch_lds<conv3d_zrw_kernel<NB>>(grid, dim3(256), ZrLds<NB, TD>::bytes(), st, p, c.segs, c.tps);
}

// A persistent form of this kernel (tile ranges per workgroup, cross-tile prefetch, like conv3d_persist_kernel) was
// built and measured: 5-20 % SLOWER on every layer of the benchmark net - <2, 8> does not fit 256 VGPRs next to the
// prefetch registers, <2, 4> loses the operand reuse - so one tile per workgroup it stays.
// Round 2 rebuilt it with what had been learnt since (scale / shift in SGPRs, tables re-derived per tile: 255 VGPRs,
// 36 B of scratch; the next tile's first chunk requested before the last k-loop; the tiles of an XCD taken interleaved so
// that neighbours stay concurrent - with one contiguous range per workgroup it lost 11-17 % per layer to L2 misses on the
// shared halos): bit-identical, its stamps show 33.7 k cycles per 2-chunk tile instead of ~43 k, and it is still 3-9 %
// slower per layer in back-to-back launches (959 vs 899 us on 32 -> 32), with or without a half-period start delay for
// the workgroup in the odd wave slot.  Requesting one dword per 128-byte line of a later tile's halo (tile + 16 .. 256
// of the XCD's range) to warm L2 / the Infinity Cache: 2-3 % slower at every distance.  Timing-only builds (-DFNN_TMODE,
// tools/zr_tmode.py) say where the time of the 32 -> 32 layer is: halo loads hitting one line -23 %, weight loads
// hitting one element -5 %, stores dropped -14 %, all three -32 %, no normalisation 0 %; MFMA work alone would be 30 %
// of the kernel's time.
// <4, 8> (four cout blocks per workgroup: the halo of a Cout >= 64 layer staged once per 64 channels instead of per 32;
// 99 KB of LDS, one workgroup per CU, one wave per SIMD with 392-456 registers, compiler-scheduled LDS reads): per layer
// 64 -> 64 392 -> 435 us, 128 -> 64 820 -> 765, 128 -> 128 265 -> 293, 256 -> 128 537 -> 561; +3.5 % conv time end to end.
// One wave per SIMD has nobody to cover its commit phases and LDS latencies; it would need a hand-pipelined k-loop.
// Round 2, also measured and dropped: (1) two tiles per 512-thread workgroup forced half a period apart (one half in its
// k-loop while the other stages, shared barriers; same registers and LDS per tile, bit-identical results): 6 % slower
// end to end than two independent workgroups per CU - a chunk's staging (load issue + normalise + LDS writes) takes
// longer than its k-loop, so the forced alternation idles the matrix cores where independent workgroups drift;
// (2) s_setprio(1) around the MFMA clusters: -0.6 %.
// Round 2, second session, the persistent form once more with what conv3d_zsp_kernel had taught (no hoisted tables: LDS
// offsets packed two per register and decoded per tile, weight addresses rebuilt per chunk; last chunk peeled so that its
// stores are unconditional; tiles of an XCD interleaved; first chunk of the next tile requested before the last k-loop;
// a plane-outer k-loop with 32 live operand registers; 255 VGPRs, one 8-byte scratch reload per tile; bit-identical):
// 32 -> 32 733 -> 783 us, 64 -> 64 348 -> 416, 128 -> 64 647 -> 757, 64 -> 32 1270 -> 1447 - 7-14 % SLOWER per layer, most
// on the layers with the most chunks, where the walk saves the least: what it loses is in the chunk loop itself.  With
// one tile per workgroup the dispatcher starts a workgroup whenever one ends, and the two workgroups of a CU drift into
// complementary phases; two walkers that start together stay together.  The single-chunk strided layer is the
// exception (conv3d_zsp_kernel, +25 %): there the serial chain IS the tile.
// Round 3, on the kernel with column-per-thread staging (all bit-identical unless marked; per-layer times from 30 back-to-back
// launches, tools/layer_time.py):
// * the k-loop's matrix work as v_mfma_f32_32x32x16_f16 with 27 exact k-steps (108 instead of 240 MFMAs per chunk and
//   wave, -10 % matrix cycles, same LDS reads; timing-only): 32 -> 32 875 -> 882 us, 64 -> 32 1489 -> 1526: neither the
//   MFMA count nor the zero-padded tap slot is what this kernel waits for;
// * two tiles per 512-thread workgroup IN PHASE (shared barriers, own LDS images - the lock-step a shared-weights
//   8-wave design would run in): 796 -> 915 us, 1390 -> 1491, 397 -> 443: independent workgroups overlap each other's
//   staging, lock-step does not;
// * TD = 4 at three workgroups per CU (141 registers, 53.8 KB): 767 -> 928 us;
// * runs of 2 .. 20 d-tiles per workgroup with (tile, chunk) as one sequence of stages - every k-loop carries the next
//   stage's loads, a tile's epilogue runs behind the staging of its successor's first chunk (245 registers, no scratch):
//   788 -> 770 us at 5 and 10 tiles, 1359 -> 1342: the other workgroup of the CU already hides what this hides; not kept;
// * PMC per wave and two-chunk tile (tools/pmc_layer.sh): 480 MFMAs = 7.7 k cycles, ~1280 other vector instructions
//   before / ~900 after the staging rewrite, 417 scalar, 202 LDS; SQ_WAIT_ANY 15 % of the wave's life, issue stalls
//   48 %, matrix pipe busy 50 -> 55 %; clock under 30 back-to-back launches 1.80 GHz, inside the network 2.13 GHz.
// Round 10: the paired order (FNN_PACK_ZRP) on conv3d_zr_kernel<NB, TD, 8> - 27 instead of 30 k-steps per two chunks.
// v_mfma_f32_16x16x16_f16 issues in the cycles of 16x16x32 (tools/mfma_rate_probe.cpp: 17.3 vs 17.2 per SIMD), so the padded
// half k-step could not simply be issued at K = 16; the saving needs the second chunk's tap 8 in the other k-half.
// Runs the layer on the kernel zr_choose chose; the weights are packed as FNN_PACK_ZR (FNN_PACK_ZRP: conv3d_zr_kernel).
int launch_conv3d_zr(ConvParams p, const ConvChoice &c, hipStream_t st) {
    const int nb = c.t[0], td = c.t[1];
    switch (c.kernel) {
        case CK_ZS: case CK_ZSP: case CK_ZSW: return launch_zs(p, c, st);
        case CK_ZR8:
            if (nb == 2) return td == 8 ? launch_zr8<2, 8>(p, st) : launch_zr8<2, 4>(p, st);
            return td == 8 ? launch_zr8<1, 8>(p, st) : launch_zr8<1, 4>(p, st);
        case CK_ZQ12: return launch_conv3d_zq12(p, st);
        case CK_ZR12: return launch_zr12<4>(p, st);
        case CK_ZRW: return nb == 2 ? launch_zrw<2>(p, c, st) : launch_zrw<1>(p, c, st);
        case CK_ZR:
            if (c.t[2] == 6) return launch_zr<2, 10, 6>(p, st);
            if (nb == 2) return td == 8 ? launch_zr<2, 8>(p, st) : launch_zr<2, 4>(p, st);
            return td == 8 ? launch_zr<1, 8>(p, st) : launch_zr<1, 4>(p, st);
    }
    return -1;
}
