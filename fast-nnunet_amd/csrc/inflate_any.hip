// inflate_any.hip - the kernels of fnn_inflate_find_blocks and fnn_inflate_stream (their host code is csrc/inflate.hip's): a
// raw deflate stream that nobody cut into segments, inflated speculatively and block-parallel, gfx950, wave64.  The rule is
// inflate_any_core.h; the register window, the CRC and the tables of a dynamic block are inflate_wave.h's and
// inflate_dyn_wave.h's, as in the segment routes.  Every phase is a launch of its own; no kernel waits on another workgroup.
//
//   inflate_any_mark_kernel     one wave per slice of 2 KiB of the input, staged in LDS with the 16 bytes behind it: every
//                               lane tests one bit position with inf_any_maybe (4 LDS dwords, no table), the survivors of
//                               a ballot are checked one after the other with the wave-uniform table header code, and the
//                               slice leaves one 64-bit mask per 64 bit positions and its count
//   inflate_any_scan_kernel     one wave: the slices' counts -> where each slice's candidates begin, and the total
//   inflate_any_write_kernel    one wave per slice: lane l owns masks 4 l .. 4 l + 3, a wave scan of their populations gives
//                               its place, and it writes its positions - compacted, ascending, without an atomic cursor
//   inflate_any_count_kernel    one wave per candidate: decodes the member without keeping an entry and records its end
//                               bit, 64-bit length, reason and reach; whether a block's end is a candidate is a binary
//                               search in the sorted positions
//   inflate_any_emit_kernel     one wave per chain member: decodes into a ring of the last 32 Ki 16-bit entries in LDS and
//                               streams the finished part of it to the member's place in the work buffer
//   inflate_any_window_kernel   one workgroup walks the members in chain order and writes the 32 KiB of resolved bytes that
//                               precede each: the dependency is serial, so it is a loop inside one workgroup
//   inflate_any_resolve_kernel  one wave per 16 KiB of the output, 256 bytes per lane: entries and windows in, bytes out,
//                               and the tile's CRC-32 folded from the lanes' as df_wave_crc does
//
// The ring (emit).  The entry of absolute output position a (the member's offset + its own position) lies at ring slot
// a % 32768, so the ring's 16-byte vectors are the aligned 16-byte vectors of the work buffer and a flush is whole vectors
// but for a member's two ends, which go singly - no wave writes an entry of another member.  A match source lies at most
// 32768 positions back, which is the ring's size: lane i of a match reads position pos - dist + i and writes pos + i; a
// slot it writes held position pos + i - 32768 <= its own source, and the lanes of one round read before any of them
// writes, so no source is lost.  The ring is flushed once 16384 entries are pending, which is tested in front of every
// sink call (a call adds at most 258), so a position is in the work buffer long before its slot is written again.  Match
// sources are never read back from global memory.
//
// LDS: the mark kernel 2064 B + the tables' 1408 B; the count kernel the tables alone; the emit kernel 65 536 B (ring) +
// 1408 B = 66 944 B: two workgroups of one wave per CU by the 160 KiB of LDS, which is this kernel's occupancy (its
// decode is a serial chain of scalar work and LDS round trips; the other member waves of the chain run on other CUs).  The
// resolve kernel 1280 B.  No kernel keeps scratch: nothing per lane is indexed by a runtime value.
//
// Bounds: the stream is read through InfWindow / a staged slice, both of which answer zeros past in_bytes without touching
// memory; positions are written below `cap`; an entry is written inside the member's [off, off + len) of the work buffer,
// where the member rule keeps pos + len <= out_bytes and the chain keeps off + len <= out_bytes; a marker's index is
// masked to the window; the resolve kernel writes out[a] for a < out_bytes only.
#include "fnn_device.h"
#include "inflate_any_core.h"
#include "inflate_dyn_wave.h"

namespace {

constexpr int INF_SLICE_DW = INF_ANY_SLICE / 4 + 4;              // a slice and the 16 bytes behind it
constexpr int INF_RING = INF_ANY_WINDOW;                         // entries
constexpr int INF_FLUSH = 16384;                                 // pending entries that start a flush

static __device__ __forceinline__ InfWindow inf_window_at(const uint8_t *in, long long in_bytes, long long bit, int lane) {
    return InfWindow(in, in_bytes, (bit >> 5) * 4, lane);
}

__global__ __launch_bounds__(DF_LANES) void inflate_any_mark_kernel(const uint8_t *in, long long in_bytes, unsigned long long *masks,
                                                                   unsigned *counts) {
    __shared__ unsigned s_in[INF_SLICE_DW];
    __shared__ uint16_t s_tables[INF_TABLE_BYTES / 2];
    const int lane = threadIdx.x;
    const long long byte0 = (long long)blockIdx.x * INF_ANY_SLICE;
    {
        const InfWindow w(in, in_bytes, 0, 0);                   // (for its load(): zeros past in_bytes)
        for (int d = lane; d < INF_SLICE_DW; d += DF_LANES) s_in[d] = w.load(byte0 / 4 + d);
    }
    __syncthreads();
    const long long left = in_bytes - byte0;
    const int bits = (int)(left < INF_ANY_SLICE ? left : INF_ANY_SLICE) * 8;
    InfWaveStore store(s_tables, lane);
    unsigned count = 0;
    for (int it = 0; it < INF_ANY_SLICE * 8 / 64; ++it) {
        const int bit = it * 64 + lane;
        bool may = false;
        if (bit < bits) {
            const int dw = bit >> 5, sh = bit & 31;              // dw + 3 <= 511 + 3 < INF_SLICE_DW
            const unsigned long long lo = s_in[dw] | (unsigned long long)s_in[dw + 1] << 32, hi = s_in[dw + 2] | (unsigned long long)s_in[dw + 3] << 32;
            may = inf_any_maybe(sh ? lo >> sh | hi << (64 - sh) : lo, (unsigned)(hi >> sh));
        }
        unsigned long long mask = __ballot(may), found = 0;
        while (mask) {
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1;
            const long long p = byte0 * 8 + it * 64 + j;
            if (inf_any_candidate(inf_window_at(in, in_bytes, p, lane), p, in_bytes, store)) found |= 1ull << j;
        }
        if (blockIdx.x == 0 && it == 0) found |= 1ull;           // bit 0 is always a candidate
        if (lane == 0) masks[(long long)blockIdx.x * INF_ANY_SLICE_MASKS + it] = found;
        count += (unsigned)__popcll(found);
    }
    if (lane == 0) counts[blockIdx.x] = count;
}

__global__ __launch_bounds__(DF_LANES) void inflate_any_scan_kernel(const unsigned *counts, long long n_slices, long long *offsets,
                                                                   long long *total) {
    const int lane = threadIdx.x;
    long long carry = 0;
    for (long long base = 0; base < n_slices; base += DF_LANES) {
        const unsigned c = base + lane < n_slices ? counts[base + lane] : 0u;
        unsigned all;
        const unsigned before = df_lane_bits_before(c, lane, &all);      // (64 slices hold 2^20 bit positions at the most)
        if (base + lane < n_slices) offsets[base + lane] = carry + before;
        carry += all;
    }
    if (lane == 0) *total = carry;
}

__global__ __launch_bounds__(DF_LANES) void inflate_any_write_kernel(const unsigned long long *masks, const long long *offsets,
                                                                    long long *positions, long long cap) {
    const int lane = threadIdx.x;
    const unsigned long long *mine = masks + (long long)blockIdx.x * INF_ANY_SLICE_MASKS + 4 * lane;
    static_assert(INF_ANY_SLICE_MASKS == 4 * DF_LANES, "four masks per lane");
    unsigned long long m[4];
    unsigned cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        m[k] = mine[k];
        cnt += (unsigned)__popcll(m[k]);
    }
    long long at = offsets[blockIdx.x] + df_lane_bits_before(cnt, lane);
    const long long bit0 = (long long)blockIdx.x * INF_ANY_SLICE * 8 + (4 * lane) * 64;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        for (unsigned long long left = m[k]; left; left &= left - 1, ++at)
            if (at < cap) positions[at] = bit0 + k * 64 + __builtin_ctzll(left);
    }
}

// whether a candidate begins at `bit`: a binary search in the sorted positions, the same in every lane
struct InfAnyKnown {
    const long long *positions;
    long long n;
    __device__ __forceinline__ bool operator()(long long bit) const {
        long long lo = 0, hi = n;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (positions[mid] < bit) lo = mid + 1;
            else hi = mid;
        }
        return lo < n && positions[lo] == bit;
    }
};

__global__ __launch_bounds__(DF_LANES) void inflate_any_count_kernel(const uint8_t *in, long long in_bytes, long long out_bytes,
                                                                    const long long *positions, long long n, InfAnyRecord *rec) {
    __shared__ uint16_t s_tables[INF_TABLE_BYTES / 2];
    const int lane = threadIdx.x;
    const long long start = positions[blockIdx.x];
    InfAnyNoSink sink;
    InfWaveStore store(s_tables, lane);
    InfAnyKnown known{positions, n};
    const InfAnyRecord r = inf_any_member(inf_window_at(in, in_bytes, start, lane), start, in_bytes, out_bytes, sink, store, known);
    if (lane == 0) rec[blockIdx.x] = r;
}

// the emit pass knows where its member ends
struct InfAnyEndsAt {
    long long end;
    __device__ __forceinline__ bool operator()(long long bit) const { return bit == end; }
};

// the ring of one member (the file's header comment); `off`: the member's place in the work buffer, in entries
struct InfAnyRing {
    uint16_t *ring, *work;
    long long off, flushed;                                      // positions [0, flushed) of the member are in the work buffer
    int lane;
    __device__ __forceinline__ unsigned slot(long long pos) const { return (unsigned)(off + pos) & (INF_RING - 1); }
    // positions [flushed, upto) -> the work buffer
    __device__ __forceinline__ void store(long long upto) {
        const long long a0 = off + flushed, a1 = off + upto;
        for (long long v = (a0 & ~7LL) + 8 * lane; v < a1; v += 8 * DF_LANES) {
            if (v >= a0 && v + 8 <= a1) {
                *(u32x4 *)(work + v) = *(const u32x4 *)(ring + ((unsigned)v & (INF_RING - 1)));
            } else {
                const long long e0 = v < a0 ? a0 : v, e1 = v + 8 < a1 ? v + 8 : a1;
                for (long long e = e0; e < e1; ++e) work[e] = ring[(unsigned)e & (INF_RING - 1)];
            }
        }
        flushed = upto;
    }
    __device__ __forceinline__ void room(long long pos) {
        if (pos - flushed >= INF_FLUSH) store(pos - ((off + pos) & 7));
    }
    __device__ __forceinline__ void literal(long long pos, unsigned v) {
        room(pos);
        if (lane == 0) ring[slot(pos)] = (uint16_t)v;
    }
    __device__ __forceinline__ void raw(long long pos, unsigned w, int k) {
        room(pos);
        if (lane < k) ring[slot(pos + lane)] = (uint16_t)((w >> (8 * lane)) & 255u);
    }
    __device__ __forceinline__ void match(long long pos, int len, int dist) {
        room(pos);
        for (int i = lane; i < len; i += DF_LANES) {
            const long long src = pos - dist + (dist >= len ? i : (int)((unsigned)i % (unsigned)dist));
            ring[slot(pos + i)] = (uint16_t)inf_any_entry(src, src < 0 ? 0u : ring[slot(src)]);
        }
    }
};

__global__ __launch_bounds__(DF_LANES) void inflate_any_emit_kernel(const uint8_t *in, long long in_bytes, const InfAnyMember *members, uint16_t *work, int *made) {
    __shared__ u32x4 s_ring[INF_RING * 2 / 16];
    __shared__ uint16_t s_tables[INF_TABLE_BYTES / 2];
    const int lane = threadIdx.x;
    const InfAnyMember m = members[blockIdx.x];
    InfAnyRing sink{(uint16_t *)s_ring, work, m.off, 0, lane};
    InfWaveStore store(s_tables, lane);
    InfAnyEndsAt ends{m.end};
    // (m.len as the output's end: the member writes no entry outside its own place whatever this decode meets)
    const InfAnyRecord r = inf_any_member(inf_window_at(in, in_bytes, m.start, lane), m.start, in_bytes, m.len, sink, store, ends);
    const bool same = r.reason == FNN_INFLATE_OK && r.len == m.len && r.end == m.end;
    if (same) sink.store(r.len);
    if (lane == 0) made[blockIdx.x] = same ? 1 : 0;
}

constexpr int INF_WINDOW_THREADS = 1024;

__global__ __launch_bounds__(INF_WINDOW_THREADS) void inflate_any_window_kernel(const InfAnyMember *members, long long k,
                                                                               const uint16_t *work, uint8_t *windows) {
    for (long long m = 0; m + 1 < k; ++m) {
        const long long off = members[m].off, len = members[m].len;
        const uint8_t *before = m ? windows + (m - 1) * INF_ANY_WINDOW : nullptr;
        uint8_t *mine = windows + m * INF_ANY_WINDOW;
        for (int j = threadIdx.x; j < INF_ANY_WINDOW; j += INF_WINDOW_THREADS) {
            const long long a = off + len - INF_ANY_WINDOW + j;
            unsigned v = 0;
            if (a >= off) {
                const unsigned e = work[a];
                v = e & INF_ANY_MARK ? (before ? before[e & (INF_ANY_WINDOW - 1)] : 0u) : e;
            } else if (before) {
                v = before[j + len];                             // a < off: j + len < 32768
            }
            mine[j] = (uint8_t)v;
        }
        __syncthreads();                                         // window m is complete, and seen, before window m + 1 reads it
    }
}

__global__ __launch_bounds__(DF_LANES) void inflate_any_resolve_kernel(const uint16_t *work, const InfAnyMember *members, long long k,
                                                                      const uint8_t *windows, uint8_t *out, long long out_bytes,
                                                                      const uint32_t *x2k, uint32_t *crcs) {
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_x2k[64];
    const int lane = threadIdx.x;
    df_crc_table<DF_LANES>(s_tab, lane);
    s_x2k[lane] = x2k[lane];
    __syncthreads();
    const long long lo = (long long)blockIdx.x * DF_CHUNK + lane * DF_SEG, hi = lo + DF_SEG < out_bytes ? lo + DF_SEG : out_bytes;
    long long m = 0;
    if (lo < hi) {                                               // the last member that begins at or before `lo`
        long long a = 0, b = k;
        while (b - a > 1) {
            const long long mid = (a + b) >> 1;
            if (members[mid].off <= lo) a = mid;
            else b = mid;
        }
        m = a;
    }
    long long next = m + 1 < k ? members[m + 1].off : out_bytes;
    uint32_t crc = 0xFFFFFFFFu;
    for (long long a = lo; a < hi; a += 8) {
        const bool whole = a + 8 <= hi;
        u32x4 e = {0u, 0u, 0u, 0u};
        if (whole) e = *(const u32x4 *)(work + a);
        else
            for (int i = 0; a + i < hi; ++i) e[i >> 1] |= (unsigned)work[a + i] << (16 * (i & 1));
        unsigned long long bytes = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (a + i < hi) {
                while (a + i >= next) {
                    ++m;
                    next = m + 1 < k ? members[m + 1].off : out_bytes;
                }
                unsigned v = (e[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
                if (v & INF_ANY_MARK) v = m ? windows[(m - 1) * INF_ANY_WINDOW + (v & (INF_ANY_WINDOW - 1))] : 0u;
                v &= 255u;
                crc = s_tab[(crc ^ v) & 255u] ^ (crc >> 8);
                bytes |= (unsigned long long)v << (8 * i);
            }
        }
        if (whole) *(unsigned long long *)(out + a) = bytes;
        else
            for (int i = 0; a + i < hi; ++i) out[a + i] = (uint8_t)(bytes >> (8 * i));
    }
    const int mylen = hi > lo ? (int)(hi - lo) : 0;
    crc = df_wave_crc(mylen ? ~crc : 0u, mylen, s_x2k, lane);
    if (lane == 0) crcs[blockIdx.x] = crc;
}

}  // namespace

void inf_any_launch(int pass, unsigned n, const InfAnyArgs &a, hipStream_t st) {
    switch (pass) {
    case INF_ANY_MARK_PASS:
        hipLaunchKernelGGL(inflate_any_mark_kernel, dim3(n), dim3(DF_LANES), 0, st, a.in, a.in_bytes, a.masks, a.counts);
        fnn_note_kernel("inflate_any_mark_kernel");
        break;
    case INF_ANY_SCAN:
        hipLaunchKernelGGL(inflate_any_scan_kernel, dim3(1), dim3(DF_LANES), 0, st, a.counts, (long long)n, a.offsets, a.total);
        fnn_note_kernel("inflate_any_scan_kernel");
        break;
    case INF_ANY_WRITE:
        hipLaunchKernelGGL(inflate_any_write_kernel, dim3(n), dim3(DF_LANES), 0, st, a.masks, a.offsets, a.positions, a.cap);
        fnn_note_kernel("inflate_any_write_kernel");
        break;
    case INF_ANY_COUNT:
        hipLaunchKernelGGL(inflate_any_count_kernel, dim3(n), dim3(DF_LANES), 0, st, a.in, a.in_bytes, a.out_bytes, a.positions, (long long)n, a.rec);
        fnn_note_kernel("inflate_any_count_kernel");
        break;
    case INF_ANY_EMIT:
        hipLaunchKernelGGL(inflate_any_emit_kernel, dim3(n), dim3(DF_LANES), 0, st, a.in, a.in_bytes, a.members, a.work, a.made);
        fnn_note_kernel("inflate_any_emit_kernel");
        break;
    case INF_ANY_WINDOW_PASS:
        hipLaunchKernelGGL(inflate_any_window_kernel, dim3(1), dim3(INF_WINDOW_THREADS), 0, st, a.members, (long long)n, a.work, a.windows);
        fnn_note_kernel("inflate_any_window_kernel");
        break;
    default:
        hipLaunchKernelGGL(inflate_any_resolve_kernel, dim3((unsigned)((a.out_bytes + DF_CHUNK - 1) / DF_CHUNK)), dim3(DF_LANES), 0, st, a.work,
                           a.members, (long long)n, a.windows, a.out, a.out_bytes, a.x2k, a.crcs);
        fnn_note_kernel("inflate_any_resolve_kernel");
    }
}
