// inflate_wave.h - what the kernels of csrc/inflate.hip, csrc/inflate_dyn.hip and csrc/inflate_any.hip share: the stream as a
// register window, the wave's LDS image of a segment, the CRC-32 and the store of a finished image, the records the passes
// leave, and how the host code of the entries (csrc/inflate.hip) launches the kernels of csrc/inflate_dyn.hip and
// csrc/inflate_any.hip.
#pragma once
#include "deflate_wave.h"
#include "inflate_core.h"
#include <hip/hip_runtime.h>

constexpr int INF_PIECE = 260;                   // the bytes of the image one lane takes the CRC of: 65 dwords, an odd pitch
static_assert(INF_PIECE % 4 == 0 && DF_LANES * INF_PIECE >= 15 + FNN_INFLATE_SEGMENT_MAX, "64 pieces cover the image");

struct InfMember {                               // a member of the chain: where its segment starts, where its bytes go
    long long start, off;
};
struct InfMade {                                 // what the emit pass says of a member
    uint32_t crc;
    int len;                                     // the bytes stored; -1: the second decode was refused (never, for the same input)
};

// the stream as a window of 64 dwords, one per lane; everything but `cur` and `nxt` is wave-uniform
struct InfWindow {
    const uint8_t *in;
    long long in_bytes, next_dw;                 // the dword index of the window after `nxt`
    unsigned cur, nxt;
    int idx, lane;
    // dword `dw` of the stream, bytes from in_bytes on as 0 (and not loaded)
    __device__ __forceinline__ unsigned load(long long dw) const {
        const long long at = dw * 4;
        if (at + 4 <= in_bytes) return *(const unsigned *)(in + at);
        unsigned w = 0;
        for (int k = 0; k < 4; ++k)
            if (at + k < in_bytes) w |= (unsigned)in[at + k] << (8 * k);
        return w;
    }
    __device__ __forceinline__ InfWindow(const uint8_t *in_, long long in_bytes_, long long start, int lane_)
        : in(in_), in_bytes(in_bytes_), idx(0), lane(lane_) {
        const long long dw = start >> 2;
        cur = load(dw + lane);
        nxt = load(dw + DF_LANES + lane);
        next_dw = dw + 2 * DF_LANES;
    }
    __device__ __forceinline__ unsigned next() {
        if (idx == DF_LANES) {
            cur = nxt;
            nxt = load(next_dw + lane);
            next_dw += DF_LANES;
            idx = 0;
        }
        const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)cur, __builtin_amdgcn_readfirstlane(idx));
        ++idx;
        return w;
    }
};

// the wave's image of the segment in LDS: position p of the output at img[p]
struct InfImage {
    uint8_t *img;
    int lane;
    __device__ __forceinline__ void literal(int pos, unsigned v) {
        if (lane == 0) img[pos] = (uint8_t)v;
    }
    __device__ __forceinline__ void raw(int pos, unsigned w, int k) {
        if (lane < k) img[pos + lane] = (uint8_t)(w >> (8 * lane));
    }
    // The source bytes [pos - dist, pos) are complete before the match begins and none of them is written by it, so the
    // lanes need no order among themselves; the wave's LDS accesses are served in program order, so the stores of the
    // tokens before are seen.
    __device__ __forceinline__ void match(int pos, int len, int dist) {
        const uint8_t *src = img + pos - dist;
        if (dist >= len) {
            for (int i = lane; i < len; i += DF_LANES) img[pos + i] = src[i];
        } else if (dist == 1) {
            const uint8_t v = src[0];
            for (int i = lane; i < len; i += DF_LANES) img[pos + i] = v;
        } else {
            for (int i = lane; i < len; i += DF_LANES) img[pos + i] = src[(unsigned)i % (unsigned)dist];
        }
    }
};

// The finished image of a member that made `len` bytes -> their CRC-32 in made[blockIdx.x] and the bytes at dst.  The CRC of
// image bytes [mis, mis + len): lane l takes those of [260 l, 260 l + 260), dword by dword (65 dwords: lane l's dword i lies
// on bank (l + i) % 32); the image goes out by aligned 16-byte vectors, the ends singly.  s_tab, s_x2k: df_crc_table's table
// and the CRC field's powers, in LDS, complete (a barrier lies between their making and this).
static __device__ __forceinline__ void inf_wave_finish(uint8_t *dst, int mis, int len, const u32x4 *s_img, const uint32_t *s_tab,
                                                       const uint32_t *s_x2k, InfMade *made, int lane) {
    const int lo = max(mis, lane * INF_PIECE), hi = min(mis + len, (lane + 1) * INF_PIECE);
    uint32_t crc = 0xFFFFFFFFu;
    const unsigned *words = (const unsigned *)s_img;
    for (int w = lo >> 2; w * 4 < hi; ++w) {
        unsigned v = words[w];
#pragma unroll
        for (int k = 0; k < 4; ++k, v >>= 8) {
            const int p = w * 4 + k;
            if (p >= lo && p < hi) crc = s_tab[(crc ^ v) & 255u] ^ (crc >> 8);
        }
    }
    const int mylen = hi > lo ? hi - lo : 0;
    crc = df_wave_crc(mylen ? ~crc : 0u, mylen, s_x2k, lane);
    if (lane == 0) made[blockIdx.x] = InfMade{crc, len};
    df_wave_store(dst, mis, len, (mis + len + 15) / 16, s_img, lane);
}

// pass 0: inflate_dyn_count_kernel over `n` candidates (starts -> rec), pass 1: inflate_dyn_emit_kernel over `n` members
// (members, x2k -> out, made); one wave each.  Host only.
struct InfDynArgs {
    const uint8_t *in;
    long long in_bytes;
    const long long *starts;
    InfRecord *rec;
    const InfMember *members;
    const uint32_t *x2k;
    uint8_t *out;
    InfMade *made;
};
void inf_dyn_launch(int pass, unsigned n, const InfDynArgs &a, hipStream_t st);

// ---- fnn_inflate_find_blocks, fnn_inflate_stream: the passes of csrc/inflate_any.hip ----------------------------------------
struct InfAnyRecord;
constexpr int INF_ANY_SLICE = 2048;                              // the input bytes of one workgroup of the block finder
constexpr int INF_ANY_SLICE_MASKS = INF_ANY_SLICE * 8 / 64;      // its 64-bit masks: one bit per bit position
struct InfAnyMember {                                            // a member of the chain: its first bit, where its entries go (in
    long long start, off, end, len;                              // entries: output bytes), the bit behind it and its length
};
enum { INF_ANY_MARK_PASS, INF_ANY_SCAN, INF_ANY_WRITE, INF_ANY_COUNT, INF_ANY_EMIT, INF_ANY_WINDOW_PASS, INF_ANY_RESOLVE };
struct InfAnyArgs {
    const uint8_t *in;
    long long in_bytes, out_bytes;
    unsigned long long *masks;                                   // per slice INF_ANY_SLICE_MASKS
    unsigned *counts;                                            // per slice
    long long *offsets, *total;                                  // per slice; one
    long long *positions, cap;                                   // the candidates, ascending; how many `positions` holds
    InfAnyRecord *rec;                                           // per candidate
    const InfAnyMember *members;
    uint16_t *work;                                              // one entry per output byte
    int *made;                                                   // per member: 1, or 0 where the second decode differed (never)
    uint8_t *windows;                                            // per member but the last, 32 KiB
    const uint32_t *x2k;
    uint8_t *out;
    uint32_t *crcs;                                              // per DF_CHUNK of the output
};
// MARK_PASS, WRITE: n slices; SCAN: n slices in one wave; COUNT: n candidates; EMIT, WINDOW_PASS, RESOLVE: n members.  Host only.
void inf_any_launch(int pass, unsigned n, const InfAnyArgs &a, hipStream_t st);
