// deflate_wave.h - what one wave of DF_LANES lanes does with its lanes' segments (deflate_core.h), device only: the steps
// the count and emit kernels of csrc/deflate.hip, csrc/deflate_dyn.hip and csrc/deflate_masks.hip are made of.  `lane`: the
// lane's index in its wave.
#pragma once
#include "deflate_core.h"
#include <hip/hip_runtime.h>

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// the 16-byte vectors of a wave's bit buffer: a chunk of up to `max_bytes` behind up to 15 bytes of its predecessor
constexpr int DF_OUT_VECS(int max_bytes) { return (15 + max_bytes + 15) / 16; }

// the 256-entry byte table of the CRC, built by THREADS threads: 256 / THREADS neighbouring entries each, one store
template <int THREADS> static __device__ __forceinline__ void df_crc_table(uint32_t *s_tab, int tid) {
#pragma unroll
    for (int k = 0; k < 256 / THREADS; ++k) {
        uint32_t t = tid * (256 / THREADS) + k;
        for (int i = 0; i < 8; ++i) t = (t >> 1) ^ ((t & 1) ? DF_POLY : 0u);
        s_tab[tid * (256 / THREADS) + k] = t;
    }
}

// ---- a chunk of a label map -> LDS (csrc/deflate.hip, csrc/deflate_dyn.hip) -------------------------------------------
// the file bytes [16 v, 16 v + 16) of chunk `c`, bytes past `len` (the chunk's length) as 0
template <bool NARROW>
static __device__ __forceinline__ u32x4 load_vec(const uint8_t *in, long long c, int v, int len) {
    const int b0 = v * 16;
    u32x4 d = {0u, 0u, 0u, 0u};
    if (!NARROW) {
        const uint8_t *p = in + c * DF_CHUNK + b0;
        if (b0 + 16 <= len) return *(const u32x4 *)p;
        for (int j = 0; b0 + j < len; ++j) d[j >> 2] |= (unsigned)p[j] << ((j & 3) * 8);
    } else {
        const uint16_t *p = (const uint16_t *)in + c * DF_CHUNK + b0;
        if (b0 + 16 <= len) {
            const u32x4 lo = ((const u32x4 *)p)[0], hi = ((const u32x4 *)p)[1];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                d[k] = (lo[2 * k] & 255u) | ((lo[2 * k] >> 8) & 0xFF00u) | ((lo[2 * k + 1] & 255u) << 16) | ((lo[2 * k + 1] & 0xFF0000u) << 8);
                d[2 + k] = (hi[2 * k] & 255u) | ((hi[2 * k] >> 8) & 0xFF00u) | ((hi[2 * k + 1] & 255u) << 16) | ((hi[2 * k + 1] & 0xFF0000u) << 8);
            }
            return d;
        }
        for (int j = 0; b0 + j < len; ++j) d[j >> 2] |= ((unsigned)p[j] & 255u) << ((j & 3) * 8);
    }
    return d;
}

// chunk `c` of the file bytes -> s_in, segment s at dword s * DF_PITCH; -> the chunk's length in bytes
template <bool NARROW>
static __device__ __forceinline__ int load_chunk(const uint8_t *in, long long n_bytes, long long c, unsigned *s_in) {
    const long long left = n_bytes - c * DF_CHUNK;
    const int len = left < DF_CHUNK ? (int)left : DF_CHUNK;
    const int vecs = (len + 15) / 16;
    for (int v = threadIdx.x; v < vecs; v += DF_LANES) {
        const u32x4 d = load_vec<NARROW>(in, c, v, len);
        unsigned *q = s_in + (v >> 4) * DF_PITCH + (v & 15) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = d[k];
    }
    return len;
}

// the bytes of the lane's segment in a chunk of `chunk_len`
static __device__ __forceinline__ int df_seg_len(int chunk_len, int lane) {
    const int l = chunk_len - lane * DF_SEG;
    return l < 0 ? 0 : (l > DF_SEG ? DF_SEG : l);
}

// the bits of all lanes, in every lane
static __device__ __forceinline__ unsigned df_wave_sum(unsigned bits) {
    for (int s = 32; s > 0; s >>= 1) bits += (unsigned)__shfl_xor((int)bits, s);
    return bits;
}

// the CRCs of the lanes' segments (`mylen` bytes each) -> the chunk's, in lane 0.
// In step s lane l takes over lanes l .. l + 2 s - 1: its own bytes, then those of lane l + s.
static __device__ __forceinline__ uint32_t df_wave_crc(uint32_t crc, int mylen, const uint32_t *s_x2k, int lane) {
    for (int s = 1; s < DF_LANES; s <<= 1) {
        const uint32_t ocrc = (uint32_t)__shfl_down((int)crc, s);
        const int olen = __shfl_down(mylen, s);
        if ((lane & (2 * s - 1)) == 0 && olen > 0) {
            crc = df_mulmod(crc, df_xpow8((unsigned long long)olen, s_x2k)) ^ ocrc;   // (a chain of segments: never DF_CHUNK bytes)
            mylen += olen;
        }
    }
    return crc;
}

// the lanes' bit counts -> the bits of the lanes before this one and, where asked for, the bits of all lanes
static __device__ __forceinline__ unsigned df_lane_bits_before(unsigned bits, int lane, unsigned *all_bits = nullptr) {
    unsigned incl = bits;
    for (int s = 1; s < DF_LANES; s <<= 1) {
        const unsigned up = (unsigned)__shfl_up((int)incl, s);
        if (lane >= s) incl += up;
    }
    if (all_bits) *all_bits = (unsigned)__shfl((int)incl, DF_LANES - 1);
    return incl - bits;
}

// ... -> the lane's first bit in a fixed-code chunk: lane 0 begins with the 3 bits of the block header
static __device__ __forceinline__ unsigned df_lane_first_bit(unsigned bits, int lane, unsigned *all_bits = nullptr) {
    const unsigned before = df_lane_bits_before(bits, lane, all_bits);
    return lane == 0 ? 0u : 3u + before;
}

// The wave's bit buffer `out` is laid out so that its 16-byte vectors are the aligned 16-byte vectors of the chunk's place
// in the output: the chunk's `nbytes` begin `mis` bytes into it.  It is zeroed (df_wave_zero), then, behind a barrier of
// the caller's, every lane ORs the codes of its segment in from `first_bit` on (df_wave_emit; ds_or_b32: the order of the
// lanes does not change the result, so the bytes are the same on every run), and behind another barrier stored (df_wave_store).
static __device__ __forceinline__ void df_wave_zero(u32x4 *out, int vecs, int lane) {
    for (int v = lane; v < vecs; v += DF_LANES) out[v] = (u32x4){0u, 0u, 0u, 0u};
}

template <int DIST, class Reader>
static __device__ __forceinline__ void df_wave_emit(unsigned *buf, int mis, int nbytes, unsigned first_bit, int lane, Reader rd, int len) {
    DfEmit<DIST> em(buf, (unsigned)mis * 8 + first_bit);
    if (lane == 0) em.put(2u, 3);                                // BFINAL = 0, BTYPE = 01
    df_walk<DIST>(rd, len, em);
    em.finish();
    // end-of-block, the stored block's header, its padding and its LEN are zeros, which the buffer holds; NLEN = FF FF
    if (lane < 2) {
        const int b = mis + nbytes - 2 + lane;
        atomicOr(buf + (b >> 2), 0xFFu << ((b & 3) * 8));
    }
}

// The aligned 16 bytes [lo, lo + 16) of `base` (aligned) from an image `img` (aligned, in LDS) laid out as `base`: whole
// when the `nbytes` from `mis` on cover them, else those of them byte by byte.  Nothing outside base[mis, mis + nbytes) is written.
static __device__ __forceinline__ void df_store_vec(uint8_t *base, int lo, int mis, int nbytes, const uint8_t *img) {
    if (lo >= mis && lo + 16 <= mis + nbytes) {
        *(u32x4 *)(base + lo) = *(const u32x4 *)(img + lo);
    } else {
        const int b0 = lo < mis ? mis : lo, b1 = lo + 16 < mis + nbytes ? lo + 16 : mis + nbytes;
        for (int b = b0; b < b1; ++b) base[b] = (uint8_t)(((const unsigned *)img)[b >> 2] >> ((b & 3) * 8));
    }
}

// the wave's buffer of `vecs` vectors -> the chunk at `dst`
static __device__ __forceinline__ void df_wave_store(uint8_t *dst, int mis, int nbytes, int vecs, const u32x4 *out, int lane) {
    for (int v = lane; v < vecs; v += DF_LANES) df_store_vec(dst - mis, v * 16, mis, nbytes, (const uint8_t *)out);
}
