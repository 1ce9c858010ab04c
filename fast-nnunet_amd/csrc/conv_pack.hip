// conv_pack.hip - host side of the conv kernels' packed weights: which taps share a k-step, which output channel a row of a
// cout block computes, and the loop that writes the MFMA fragment order (fp16, or e4m3 with one scale per output channel).
// Serves every conv family (FNN_PACK_*: fnn_device.h); FNN_PACK_ZP's own order is conv_zp_pack (conv2d_zp.hip).
#include "fnn_device.h"
#include <algorithm>
#include <cmath>
#include <vector>

int conv3d_ksteps(int packing, int taps) {
    return packing == FNN_PACK_ZR || packing == FNN_PACK_ZRP ? 15 : packing == FNN_PACK_ZP ? 9 : (taps + 1) / 2;
}

int conv3d_kstep_tap(int packing, int ks, int half, int taps, int ch, int chunks, int *tch) {
    *tch = ch;
    if (packing == FNN_PACK_ZR || packing == FNN_PACK_ZRP) {
        const int pr = ks / 3, dz = ks % 3;
        if (pr < 4) return dz * 9 + 2 * pr + half;
        // k-steps 12 .. 14: the leftover in-plane tap 8 - padded in FNN_PACK_ZR and in FNN_PACK_ZRP's unpaired last chunk,
        // shared by the two chunks of a pair in FNN_PACK_ZRP (in the pair's second chunk; the first chunk's are zeros)
        if (packing == FNN_PACK_ZR || (ch % 2 == 0 && ch + 1 == chunks)) return half ? -1 : dz * 9 + 8;
        if (ch % 2 == 0) return -1;
        *tch = ch - 1 + half;
        return dz * 9 + 8;
    }
    const int t = 2 * ks + half;
    return t < taps ? t : -1;
}

// Output channel that row m of cout block cb of the packed weights computes.  The ZR kernels at two cout blocks per
// workgroup (an even block count) interleave the two blocks' rows in groups of four: MFMA lane quarter q then holds
// channels q * 8 .. q * 8 + 7 of a voxel (4 from each block) = ONE 16-byte store, and four lanes cover the 64 bytes of a
// 32-channel group - half the store instructions of the 8-byte form, whole 64-byte runs (the stores of this kernel
// delayed the next workgroup's loads in the texture-address path: a timing-only build without them ran 14 % faster).
int conv3d_pack_cout(int packing, int nblk, int cb, int m) {
    if ((packing != FNN_PACK_ZR && packing != FNN_PACK_ZRP && packing != FNN_PACK_ZP) || nblk % 2 != 0) return cb * 16 + m;
    return (cb >> 1) * 32 + (m >> 2) * 8 + (cb & 1) * 4 + (m & 3);
}

size_t conv_packed_halves(const ConvChoice &c, int cout_pad) { return (size_t)(cout_pad / 16) * c.chunks * c.ksteps * 512; }

uint8_t f2e4m3(float f) {
    const uint8_t sign = std::signbit(f) ? 0x80 : 0;
    float a = std::fabs(f);
    if (!(a == a)) return sign | 0x7f;
    if (a >= 448.f) return sign | 0x7e;
    if (a < 0x1p-6f) {                                          // subnormal: multiples of 2^-9
        const int q = (int)std::nearbyint(a * 512.f);           // 0 .. 8 (8 = the smallest normal)
        return sign | (uint8_t)q;                               // q = 8 -> exponent field 1, mantissa 0 = 0x08
    }
    int e;
    const float m = std::frexp(a, &e);                          // a = m * 2^e, m in [0.5, 1)
    int q = (int)std::nearbyint(m * 16.f);                      // 8 .. 16
    int E = e - 1;                                              // a = (q / 8) * 2^E
    if (q == 16) { q = 8; ++E; }
    if (E > 8 || (E == 8 && q > 14)) return sign | 0x7e;
    return sign | (uint8_t)(((E + 7) << 3) | (q - 8));
}

// One loop over the fragment order for every packing but FNN_PACK_ZP; the element encoding is the only difference between
// fp16 and fp8 (one scale per output channel: max |w| of the channel -> 448)
void conv_pack_weights(const ConvParams &p, const ConvChoice &c, int cout_real, const int cin_real[2], const float *W, void *dst,
                       float *scales) {
    const int cin_real1 = p.n_src > 1 ? cin_real[1] : 0, cin_pad0 = p.src[0].C;
    if (c.packing == FNN_PACK_ZP) {
        conv_zp_pack(W, cout_real, p.Cout, cin_real[0], cin_pad0, cin_real1, p.n_src > 1 ? p.src[1].C : 0, (unsigned short *)dst);
        return;
    }
    const int T = p.kd * p.kh * p.kw, cin_tot = cin_real[0] + cin_real1, nblk = p.Cout / 16;
    std::vector<float> inv(p.Cout, 1.f);
    if (p.fp8)
        for (int co = 0; co < p.Cout; ++co) {
            float mx = 0.f;
            if (co < cout_real)
                for (size_t i = 0; i < (size_t)cin_tot * T; ++i) mx = std::max(mx, std::fabs(W[(size_t)co * cin_tot * T + i]));
            float ws = mx / 448.f, iv = 1.f / ws;
            // an all-zero cout, or one whose max |w| < ~1.3e-36 makes ws subnormal and 1 / ws infinite (0 * inf = NaN): zero
            // weights, as the fp16 encoding rounds them
            if (!(mx > 0.f) || !std::isfinite(iv)) { ws = 1.f; iv = 0.f; }
            inv[co] = iv;
            scales[co] = ws / FNN_FP8_ACT_MULT;
        }
    for (int cb = 0; cb < nblk; ++cb)
        for (int ch = 0; ch < c.chunks; ++ch)
            for (int ks = 0; ks < c.ksteps; ++ks)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int k = 8 * (lane >> 4) + j;
                        int tch;
                        const int tap = conv3d_kstep_tap(c.packing, ks, k >> 4, T, ch, c.chunks, &tch), ci = tch * 16 + (k & 15);
                        const int co = conv3d_pack_cout(c.packing, nblk, cb, lane & 15);
                        const int src = ci >= cin_pad0, cl = src ? ci - cin_pad0 : ci;
                        float v = 0.f;
                        if (tap >= 0 && co < cout_real && cl < (src ? cin_real1 : cin_real[0]))
                            v = W[((size_t)co * cin_tot + (src ? cin_real[0] : 0) + cl) * T + tap] * inv[co];
                        const size_t i = ((((size_t)cb * c.chunks + ch) * c.ksteps + ks) * 64 + lane) * 8 + j;
                        if (p.fp8) ((uint8_t *)dst)[i] = f2e4m3(v);
                        else ((unsigned short *)dst)[i] = fnn_half_bits(v);
                    }
}
