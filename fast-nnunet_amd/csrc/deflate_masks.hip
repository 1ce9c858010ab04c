// deflate_masks.hip - a label map on the device -> one raw-deflate fragment per requested label, of the uint8 mask
// m[i] = (seg[i] == l), gfx950.  The mask files of a case (JHUPredictor: <case>/predictions/<label_name>.nii.gz) in one
// pass over the map per phase instead of one encoder run per label.
//
//   fnn_deflate_masks_count   sizes and CRC-32s of all fragments; what it found stays in `work`
//   fnn_deflate_masks_emit    the fragments, one behind the other
//
// The stream format is deflate.hip's (deflate_core.h; the steps of a wave: deflate_wave.h) over the mask bytes, with the one
// change stated there: a full chunk in which the label does not occur is the constant zero chunk.  A 16 KiB piece of an
// anatomical label map holds very few labels, so nearly every (chunk, label) pair is that constant, and the walk work
// follows the pairs whose label occurs.
//
//   deflate_masks_count_kernel<E>   one workgroup (4 waves) per chunk: the chunk's labels of E bytes -> LDS with 16-byte loads,
//                                   marking a bitset by value on the way.  Per requested label that occurs (and for every
//                                   label in a last partial chunk) one wave walks the chunk comparing on read
//                                   (DfMask: no mask bytes are stored) -> the pair's bytes (2 B) and CRC-32.  Pairs
//                                   whose label is absent are not touched: their size stays 0 = "zero chunk".
//   deflate_masks_scan_kernel       one workgroup per label: the sizes of its chunks -> their offsets in its fragment, the
//                                   fragment's size, and the fold of the chunks' CRCs (the zero chunk's term is a constant).
//   deflate_masks_emit_kernel<E>    the chunk and the bitset again (2 waves).  Absent labels: the 112 constant bytes, 8 lanes
//                                   per pair, from a table that holds the constant at each of the 16 alignments: an image
//                                   that df_store_vec takes like a bit buffer.  Present labels: a wave walks twice - the
//                                   bits per lane, then the codes into its bit buffer - and stores as deflate_emit_kernel.
//
// LDS.  A segment of 256 labels lies at a pitch of 64 E + 1 dwords (odd: the lanes' walks fall on different banks), so
// the chunk takes 16.25 KiB (E = 1) or 32.25 KiB (E = 2); the bitset 32 B or 8 KiB.  count: + the CRC table 1 KiB, the
// powers 256 B, the list of present labels 1 KiB = 18.6 KiB / 42.6 KiB, static.  emit: + the alignment table 2 KiB, the
// list 0.5 KiB and per wave a bit buffer of DF_OUT_VECS(DF_MASK_CHUNK_MAX_BYTES) vectors = 16.03 KiB: with two waves
// 50.9 KiB / 74.9 KiB, dynamic (three / two workgroups per CU).  deflate.hip's layout - a padded image of the mask bytes
// per wave next to its bit buffer - would need 34.6 KiB per wave on top of the chunk.
// Nothing is written outside out[0, sum of the fragment sizes); no kernel keeps scratch.
#include "host_call.h"
#include "deflate_wave.h"
#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

constexpr int MK_COUNT_WAVES = 4, MK_COUNT_THREADS = MK_COUNT_WAVES * DF_LANES;
constexpr int MK_EMIT_WAVES = 2, MK_EMIT_THREADS = MK_EMIT_WAVES * DF_LANES;
constexpr int MK_SCAN_THREADS = 1024;
constexpr int MK_OUT_VECS = DF_OUT_VECS(DF_MASK_CHUNK_MAX_BYTES);         // a wave's bit buffer
constexpr int MK_MAX_LABELS = 65536;                                      // every value of a 2-byte label once
constexpr int MK_ZERO_PITCH = 128;                                        // the zero chunk behind up to 15 bytes, in whole vectors

template <int E> struct MkLayout {
    static constexpr int PITCH = DF_SEG * E / 4 + 1;                      // dwords between two segments
    static constexpr int IN_DW = DF_LANES * PITCH;                        // a multiple of 4 for E = 1 and 2
    static constexpr int BITS_DW = E == 1 ? 8 : 2048;                     // one bit per value
    static constexpr unsigned VALUES = E == 1 ? 256u : 65536u;
    static constexpr int EMIT_LDS = (IN_DW + BITS_DW) * 4 + 16 * MK_ZERO_PITCH + MK_EMIT_THREADS * 4 + 16 + MK_EMIT_WAVES * MK_OUT_VECS * 16;
};
static_assert(MkLayout<1>::IN_DW % 4 == 0 && MkLayout<2>::IN_DW % 4 == 0, "the parts behind the chunk stay 16-byte aligned");

// `work`: what count leaves for emit
struct MkWork {
    size_t o_x2k, o_zero, o_labels, o_frag, o_fbytes, o_fcrc, o_slots, o_sizes, total;
    MkWork(long long n_elems, int n_labels) {
        const size_t L = (size_t)n_labels, pairs = L * (size_t)((n_elems + DF_CHUNK - 1) / DF_CHUNK);
        o_x2k = 0;                                       // x^(2^k) modulo the CRC polynomial, 64 x 4 B
        o_zero = 256;                                    // the zero chunk, 112 B in 128
        o_labels = o_zero + 128;                         // the labels, 4 B each
        o_frag = o_labels + df_align16(4 * L);           // where each fragment begins in `out`, and the end of the last: 8 B each
        o_fbytes = o_frag + df_align16(8 * (L + 1));     // the fragments' sizes, 8 B each
        o_fcrc = o_fbytes + df_align16(8 * L);           // their CRCs, 4 B each
        o_slots = o_fcrc + df_align16(4 * L);            // per (label, chunk): the chunk's CRC, then its offset in the fragment, 8 B
        o_sizes = o_slots + 8 * pairs;                   // per (label, chunk): the chunk's bytes, 0 = the zero chunk, 2 B
        total = o_sizes + df_align16(2 * pairs);
    }
};

struct MkTables : DfTables {
    uint8_t zero[128];                                   // the zero chunk
    uint32_t zero_crc;                                   // zlib's CRC-32 of DF_CHUNK zero bytes
    MkTables() {
        memset(zero, 0, sizeof(zero));
        df_zero_chunk(zero);
        uint32_t c = 0xFFFFFFFFu;
        for (int i = 0; i < DF_CHUNK * 8; ++i) c = (c >> 1) ^ ((c & 1) ? DF_POLY : 0u);
        zero_crc = ~c;
    }
};
static const MkTables g_tables;

// chunk `c` of the map -> s_in (segment s at dword s * PITCH), every value met marked in s_bits (zeroed before);
// -> the chunk's length in elements.  Nothing past element n is read.
template <int E, int THREADS>
static __device__ __forceinline__ int load_chunk_and_mark(const uint8_t *in, long long n, long long c, unsigned *s_in, unsigned *s_bits) {
    typedef MkLayout<E> Lay;
    constexpr int PER_VEC = 16 / E, SEG_VECS = DF_SEG / PER_VEC;
    const long long left = n - c * DF_CHUNK;
    const int len = left < DF_CHUNK ? (int)left : DF_CHUNK;
    const int vecs = (len + PER_VEC - 1) / PER_VEC;
    const uint8_t *base = in + c * DF_CHUNK * E;
    for (int v = threadIdx.x; v < vecs; v += THREADS) {
        const int e0 = v * PER_VEC, valid = len - e0 < PER_VEC ? len - e0 : PER_VEC;
        u32x4 d = {0u, 0u, 0u, 0u};
        if (valid == PER_VEC) d = *(const u32x4 *)(base + (size_t)v * 16);
        else
            for (int j = 0; j < valid * E; ++j) d[j >> 2] |= (unsigned)base[(size_t)v * 16 + j] << ((j & 3) * 8);
        unsigned *q = s_in + (v / SEG_VECS) * Lay::PITCH + (v % SEG_VECS) * 4;
        unsigned prev = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            q[k] = d[k];
#pragma unroll
            for (int j = 0; j < 4 / E; ++j) {
                const unsigned val = E == 1 ? (d[k] >> (8 * j)) & 255u : (d[k] >> (16 * j)) & 0xFFFFu;
                if (k * (4 / E) + j < valid && val != prev) { atomicOr(s_bits + (val >> 5), 1u << (val & 31)); prev = val; }
            }
        }
    }
    return len;
}

template <int E> static __device__ __forceinline__ bool occurs(const unsigned *s_bits, int label) {
    return (unsigned)label < MkLayout<E>::VALUES && ((s_bits[label >> 5] >> (label & 31)) & 1u);
}

template <int E>
__global__ __launch_bounds__(MK_COUNT_THREADS) void deflate_masks_count_kernel(const uint8_t *in, long long n, const int32_t *labels, int n_labels,
                                                                                const uint32_t *x2k, long long chunks, uint16_t *sizes,
                                                                                unsigned long long *slots) {
    typedef MkLayout<E> Lay;
    __shared__ unsigned s_in[Lay::IN_DW];
    __shared__ unsigned s_bits[Lay::BITS_DW];
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_x2k[64];
    __shared__ int s_list[MK_COUNT_THREADS];
    __shared__ int s_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long c = blockIdx.x;
    df_crc_table<MK_COUNT_THREADS>(s_tab, tid);
    if (tid < 64) s_x2k[tid] = x2k[tid];
    for (int i = tid; i < Lay::BITS_DW; i += MK_COUNT_THREADS) s_bits[i] = 0u;
    __syncthreads();
    const int len = load_chunk_and_mark<E, MK_COUNT_THREADS>(in, n, c, s_in, s_bits);
    const bool full = len == DF_CHUNK;
    for (int k0 = 0; k0 < n_labels; k0 += MK_COUNT_THREADS) {
        if (tid == 0) s_n = 0;
        __syncthreads();                                         // the chunk and the bitset are whole; the list is free
        const int k = k0 + tid;
        if (k < n_labels && (!full || occurs<E>(s_bits, labels[k]))) s_list[atomicAdd(&s_n, 1)] = k;
        __syncthreads();
        const int np = s_n;
        for (int i = wave; i < np; i += MK_COUNT_WAVES) {
            const int kk = s_list[i];
            const int mylen = df_seg_len(len, lane);
            DfCount<1> cnt{s_tab};
            df_walk<1>(DfMask<E>{s_in + lane * Lay::PITCH, (unsigned)labels[kk]}, mylen, cnt);
            const unsigned bits = df_wave_sum(cnt.bits);
            const uint32_t crc = df_wave_crc(~cnt.crc, mylen, s_x2k, lane);
            if (lane == 0) {
                sizes[(long long)kk * chunks + c] = (uint16_t)df_chunk_bytes(bits);
                slots[(long long)kk * chunks + c] = crc;
            }
        }
        __syncthreads();                                         // the list is read out before the next tile resets it
    }
}

// One workgroup per label.  slots[i]: the CRC of chunk i on entry (where sizes[i] != 0), its offset in the fragment on return.
__global__ __launch_bounds__(MK_SCAN_THREADS) void deflate_masks_scan_kernel(const uint16_t *sizes, unsigned long long *slots, long long chunks,
                                                                             int last_len, uint32_t zero_crc, const uint32_t *x2k,
                                                                             long long *frag_bytes, uint32_t *frag_crc) {
    __shared__ long long s_sum[MK_SCAN_THREADS];
    __shared__ long long s_len[MK_SCAN_THREADS];
    __shared__ uint32_t s_crc[MK_SCAN_THREADS];
    __shared__ uint32_t s_x2k[64];
    const int t = threadIdx.x;
    const uint16_t *sz = sizes + (long long)blockIdx.x * chunks;
    unsigned long long *sl = slots + (long long)blockIdx.x * chunks;
    if (t < 64) s_x2k[t] = x2k[t];
    __syncthreads();
    const uint32_t x_chunk = df_xpow8(DF_CHUNK, s_x2k);
    const long long per = (chunks + MK_SCAN_THREADS - 1) / MK_SCAN_THREADS;
    const long long lo = min(chunks, t * per), hi = min(chunks, lo + per);
    long long sum = 0, len = 0;
    uint32_t crc = 0;
    for (long long i = lo; i < hi; ++i) {
        const unsigned s = sz[i];
        sum += s ? s : DF_ZERO_CHUNK_BYTES;
        const int li = i == chunks - 1 ? last_len : DF_CHUNK;
        crc = df_crc_append(crc, s ? (uint32_t)sl[i] : zero_crc, (unsigned long long)li, s_x2k, x_chunk);
        len += li;
    }
    s_sum[t] = sum;
    s_len[t] = len;
    s_crc[t] = crc;
    __syncthreads();
    for (int s = 1; s < MK_SCAN_THREADS; s <<= 1) {
        const long long add = t >= s ? s_sum[t - s] : 0;
        // thread t takes over threads t .. t + 2 s - 1: its own chunks, then those of thread t + s (which does not write here)
        if ((t & (2 * s - 1)) == 0 && s_len[t + s] > 0) {
            s_crc[t] = df_crc_append(s_crc[t], s_crc[t + s], (unsigned long long)s_len[t + s], s_x2k, x_chunk);
            s_len[t] += s_len[t + s];
        }
        __syncthreads();
        s_sum[t] += add;
        __syncthreads();
    }
    long long run = s_sum[t] - sum;
    for (long long i = lo; i < hi; ++i) {
        const unsigned s = sz[i];
        sl[i] = (unsigned long long)run;
        run += s ? s : DF_ZERO_CHUNK_BYTES;
    }
    if (t == 0) frag_crc[blockIdx.x] = s_crc[0];
    if (t == MK_SCAN_THREADS - 1) frag_bytes[blockIdx.x] = s_sum[t];
}

template <int E>
__global__ __launch_bounds__(MK_EMIT_THREADS) void deflate_masks_emit_kernel(const uint8_t *in, long long n, const int32_t *labels, int n_labels,
                                                                              long long chunks, const uint16_t *sizes,
                                                                              const unsigned long long *slots, const long long *frag,
                                                                              const uint8_t *zero, uint8_t *out, long long total) {
    typedef MkLayout<E> Lay;
    extern __shared__ u32x4 s_dyn[];
    unsigned *s_in = (unsigned *)s_dyn;
    unsigned *s_bits = s_in + Lay::IN_DW;
    uint8_t *s_zero = (uint8_t *)(s_bits + Lay::BITS_DW);        // [mis][MK_ZERO_PITCH]: the zero chunk behind `mis` bytes
    int *s_list = (int *)(s_zero + 16 * MK_ZERO_PITCH);
    int *s_n = s_list + MK_EMIT_THREADS;                         // (4 ints: what follows stays 16-byte aligned)
    u32x4 *s_out = (u32x4 *)(s_n + 4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long c = blockIdx.x;
    for (int i = tid; i < Lay::BITS_DW; i += MK_EMIT_THREADS) s_bits[i] = 0u;
    for (int i = tid; i < 16 * MK_ZERO_PITCH; i += MK_EMIT_THREADS) {
        const int o = (i & (MK_ZERO_PITCH - 1)) - (i / MK_ZERO_PITCH);
        s_zero[i] = o >= 0 && o < DF_ZERO_CHUNK_BYTES ? zero[o] : (uint8_t)0;
    }
    __syncthreads();
    const int len = load_chunk_and_mark<E, MK_EMIT_THREADS>(in, n, c, s_in, s_bits);
    const bool full = len == DF_CHUNK;
    u32x4 *my_out = s_out + wave * MK_OUT_VECS;
    unsigned *buf = (unsigned *)my_out;
    for (int k0 = 0; k0 < n_labels; k0 += MK_EMIT_THREADS) {
        if (tid == 0) *s_n = 0;
        __syncthreads();                                         // the chunk, the bitset and the table are whole; the list is free
        const int k = k0 + tid;
        if (k < n_labels && (!full || occurs<E>(s_bits, labels[k]))) s_list[atomicAdd(s_n, 1)] = k;
        // absent labels: 8 lanes per pair, lane j the aligned 16 bytes j of `out` that the pair's 112 bytes touch
        const int here = n_labels - k0 < MK_EMIT_THREADS ? n_labels - k0 : MK_EMIT_THREADS;
        for (int idx = tid; full && idx < here * 8; idx += MK_EMIT_THREADS) {
            const int kk = k0 + (idx >> 3), lo = (idx & 7) * 16;
            if (occurs<E>(s_bits, labels[kk])) continue;
            const long long at = frag[kk] + (long long)slots[(long long)kk * chunks + c];
            if (at < 0 || at + DF_ZERO_CHUNK_BYTES > total) continue;     // (a `work` that count did not fill must not reach outside `out`)
            uint8_t *dst = out + at;
            const int mis = (int)((uintptr_t)dst & 15);
            df_store_vec(dst - mis, lo, mis, DF_ZERO_CHUNK_BYTES, s_zero + mis * MK_ZERO_PITCH);
        }
        __syncthreads();
        const int np = *s_n;
        for (int i0 = 0; i0 < np; i0 += MK_EMIT_WAVES) {
            const bool act = i0 + wave < np;                     // (uniform in the wave; every wave keeps the barriers)
            uint8_t *dst = out;
            int mis = 0, nbytes = 0, vecs = 0;
            unsigned label = 0, bits = 0;
            if (act) {
                const int kk = s_list[i0 + wave];
                label = (unsigned)labels[kk];
                const long long at = frag[kk] + (long long)slots[(long long)kk * chunks + c];
                nbytes = (int)sizes[(long long)kk * chunks + c];
                if (at < 0 || at + nbytes > total) nbytes = 0;   // (as above; 0 bytes never equal what the walk counts)
                dst = out + (nbytes ? at : 0);
                mis = (int)((uintptr_t)dst & 15);                // the chunk begins `mis` bytes into an aligned 16 bytes of `out`
                vecs = (mis + nbytes + 15) / 16;                 // <= MK_OUT_VECS
                if (vecs > MK_OUT_VECS) vecs = MK_OUT_VECS;      // (a `work` that count did not fill must not reach past the buffer)
                df_wave_zero(my_out, vecs, lane);
                DfCount<1, false> cnt;
                df_walk<1>(DfMask<E>{s_in + lane * Lay::PITCH, label}, df_seg_len(len, lane), cnt);
                bits = cnt.bits;
            }
            unsigned all_bits;
            const unsigned first_bit = df_lane_first_bit(bits, lane, &all_bits);
            // what the walk is about to write must be what count sized, or the buffer and `out` would be overrun
            const bool fits = act && (int)df_chunk_bytes(all_bits) == nbytes && nbytes <= DF_MASK_CHUNK_MAX_BYTES;
            __syncthreads();
            if (fits) df_wave_emit<1>(buf, mis, nbytes, first_bit, lane, DfMask<E>{s_in + lane * Lay::PITCH, label}, df_seg_len(len, lane));
            __syncthreads();
            if (fits) df_wave_store(dst, mis, nbytes, vecs, my_out, lane);
        }
        __syncthreads();                                         // the list is read out before the next tile resets it
    }
}

// what both calls refuse before they launch anything -> 0, or the code (the message is set)
static int check_common(const char *who, const void *in, int in_elem_bytes, int64_t n_elems, const int32_t *labels, int n_labels,
                        const void *work) {
    auto fail = [&](int code, const char *what) { return fnn_failf(code, "%s: %s", who, what); };
    if (!in || !labels || !work) return fail(FNN_E_INVALID, "NULL argument");
    if (in_elem_bytes != 1 && in_elem_bytes != 2) return fail(FNN_E_INVALID, "labels of 1 or 2 bytes are served");
    if (n_elems < 0) return fail(FNN_E_INVALID, "negative element count");
    if ((uintptr_t)in % 16) return fail(FNN_E_INVALID, "in must be aligned to 16 bytes");
    if ((uintptr_t)work % 16) return fail(FNN_E_INVALID, "work must be aligned to 16 bytes");
    if (n_labels < 1) return fail(FNN_E_INVALID, "n_labels must be at least 1");
    std::vector<bool> seen(MK_MAX_LABELS, false);
    for (int k = 0; k < n_labels; ++k) {
        if (labels[k] < 0 || labels[k] >= MK_MAX_LABELS) return fail(FNN_E_INVALID, "a label lies outside [0, 65535]");
        if (seen[(size_t)labels[k]]) return fail(FNN_E_INVALID, "a label is named twice (duplicate)");
        seen[(size_t)labels[k]] = true;
    }
    // one workgroup per chunk: 2^31 - 1 chunks of 16 Ki labels (65536 distinct labels at most, which the scan's grid addresses)
    if (n_elems > (int64_t)INT_MAX * DF_CHUNK) return fail(FNN_E_UNSUPPORTED, "too many elements for one launch sequence");
    return 0;
}

}  // namespace

extern "C" int64_t fnn_deflate_masks_work_bytes(int64_t n_elems, int n_labels) {
    if (n_elems < 0 || n_labels < 1 || n_labels > MK_MAX_LABELS || n_elems > (int64_t)INT_MAX * DF_CHUNK) return 0;
    return (int64_t)MkWork(n_elems, n_labels).total;
}

extern "C" int fnn_deflate_masks_count(const void *in, int in_elem_bytes, int64_t n_elems, const int32_t *labels, int n_labels,
                                       void *work, int64_t work_cap, int64_t *frag_bytes, uint32_t *crc32, void *stream) {
    FnnOpKlog klog;
    if (!frag_bytes || !crc32) return fnn_fail(FNN_E_INVALID, "fnn_deflate_masks_count: NULL argument");
    if (const int rc = check_common("fnn_deflate_masks_count", in, in_elem_bytes, n_elems, labels, n_labels, work)) return rc;
    const MkWork w(n_elems, n_labels);
    if (work_cap < (int64_t)w.total) return fnn_fail(FNN_E_INVALID, "fnn_deflate_masks_count: work_cap is below fnn_deflate_masks_work_bytes");
    if (int rc = fnn_need_dev("fnn_deflate_masks_count", {in, work}, "device pointers for in and work")) return rc;
    for (int k = 0; k < n_labels; ++k) { frag_bytes[k] = 0; crc32[k] = 0; }
    if (n_elems == 0) return FNN_OK;

    char *base = (char *)work;
    const long long chunks = (n_elems + DF_CHUNK - 1) / DF_CHUNK;
    const int last_len = (int)(n_elems - (chunks - 1) * DF_CHUNK);
    uint32_t *d_x2k = (uint32_t *)(base + w.o_x2k);
    int32_t *d_labels = (int32_t *)(base + w.o_labels);
    long long *d_frag = (long long *)(base + w.o_frag), *d_fbytes = (long long *)(base + w.o_fbytes);
    uint32_t *d_fcrc = (uint32_t *)(base + w.o_fcrc);
    unsigned long long *d_slots = (unsigned long long *)(base + w.o_slots);
    uint16_t *d_sizes = (uint16_t *)(base + w.o_sizes);
    HipCall call(stream);
    call.copy(d_x2k, g_tables.x2k, sizeof(g_tables.x2k), hipMemcpyHostToDevice);
    call.copy(base + w.o_zero, g_tables.zero, sizeof(g_tables.zero), hipMemcpyHostToDevice);
    call.copy(d_labels, labels, (size_t)n_labels * 4, hipMemcpyHostToDevice);
    call.fill(d_sizes, 0, (size_t)n_labels * (size_t)chunks * 2);                                        // every pair: the zero chunk
    if (call.ok()) fnn_note_kernel("deflate_masks_count_kernel<%d>", in_elem_bytes);
    call.launch(in_elem_bytes == 1 ? deflate_masks_count_kernel<1> : deflate_masks_count_kernel<2>, dim3((unsigned)chunks),
                dim3(MK_COUNT_THREADS), 0, (const uint8_t *)in, (long long)n_elems, d_labels, n_labels, d_x2k, chunks, d_sizes, d_slots);
    if (call.ok()) fnn_note_kernel("deflate_masks_scan_kernel");
    call.launch(deflate_masks_scan_kernel, dim3((unsigned)n_labels), dim3(MK_SCAN_THREADS), 0, d_sizes, d_slots, chunks, last_len,
                g_tables.zero_crc, d_x2k, d_fbytes, d_fcrc);
    std::vector<long long> h_bytes((size_t)n_labels), h_frag((size_t)n_labels + 1);
    call.copy(h_bytes.data(), d_fbytes, (size_t)n_labels * 8, hipMemcpyDeviceToHost);
    call.copy(crc32, d_fcrc, (size_t)n_labels * 4, hipMemcpyDeviceToHost);
    if (call.sync()) {
        h_frag[0] = 0;
        for (int k = 0; k < n_labels; ++k) { frag_bytes[k] = h_bytes[(size_t)k]; h_frag[(size_t)k + 1] = h_frag[(size_t)k] + h_bytes[(size_t)k]; }
        call.copy(d_frag, h_frag.data(), ((size_t)n_labels + 1) * 8, hipMemcpyHostToDevice);
    }
    if (!call.sync()) {
        for (int k = 0; k < n_labels; ++k) { frag_bytes[k] = 0; crc32[k] = 0; }
        return call.fail();
    }
    return FNN_OK;
}

extern "C" int fnn_deflate_masks_emit(const void *in, int in_elem_bytes, int64_t n_elems, const int32_t *labels, int n_labels,
                                      const void *work, void *out, int64_t out_cap, void *stream) {
    FnnOpKlog klog;
    if (!out) return fnn_fail(FNN_E_INVALID, "fnn_deflate_masks_emit: NULL argument");
    if (const int rc = check_common("fnn_deflate_masks_emit", in, in_elem_bytes, n_elems, labels, n_labels, work)) return rc;
    if (out_cap < 0) return fnn_fail(FNN_E_INVALID, "fnn_deflate_masks_emit: out_cap is negative");
    if (int rc = fnn_need_dev("fnn_deflate_masks_emit", {in, work, out}, "device pointers for in, work and out")) return rc;
    if (n_elems == 0) return FNN_OK;

    const MkWork w(n_elems, n_labels);
    const char *base = (const char *)work;
    const long long chunks = (n_elems + DF_CHUNK - 1) / DF_CHUNK;
    const long long *d_frag = (const long long *)(base + w.o_frag);
    hipStream_t st = (hipStream_t)stream;
    // the sizes count left: the labels and the end of the last fragment (count has synchronised; this waits for nothing new)
    std::vector<int32_t> h_labels((size_t)n_labels);
    long long total = -1;
    HipCall call(stream);
    call.copy(&total, d_frag + n_labels, 8, hipMemcpyDeviceToHost);
    call.copy(h_labels.data(), base + w.o_labels, (size_t)n_labels * 4, hipMemcpyDeviceToHost);
    if (!call.sync()) return call.fail();
    if (memcmp(h_labels.data(), labels, (size_t)n_labels * 4) != 0)
        return fnn_fail(FNN_E_INVALID, "fnn_deflate_masks_emit: work was not filled by fnn_deflate_masks_count for these labels");
    if (total < 0 || out_cap < total) return fnn_fail(FNN_E_INVALID, "fnn_deflate_masks_emit: out_cap is below the sum of the fragment sizes");
    int rc;
    if (in_elem_bytes == 1)
        rc = fnn_launch_lds<deflate_masks_emit_kernel<1>>(dim3((unsigned)chunks), dim3(MK_EMIT_THREADS), (size_t)MkLayout<1>::EMIT_LDS, st,
                                                          (const uint8_t *)in, (long long)n_elems, (const int32_t *)(base + w.o_labels), n_labels, chunks,
                                                          (const uint16_t *)(base + w.o_sizes), (const unsigned long long *)(base + w.o_slots), d_frag,
                                                          (const uint8_t *)(base + w.o_zero), (uint8_t *)out, total);
    else
        rc = fnn_launch_lds<deflate_masks_emit_kernel<2>>(dim3((unsigned)chunks), dim3(MK_EMIT_THREADS), (size_t)MkLayout<2>::EMIT_LDS, st,
                                                          (const uint8_t *)in, (long long)n_elems, (const int32_t *)(base + w.o_labels), n_labels, chunks,
                                                          (const uint16_t *)(base + w.o_sizes), (const unsigned long long *)(base + w.o_slots), d_frag,
                                                          (const uint8_t *)(base + w.o_zero), (uint8_t *)out, total);
    fnn_note_kernel("deflate_masks_emit_kernel<%d>", in_elem_bytes);
    if (rc != 0) return fnn_fail(FNN_E_HIP, "fnn_deflate_masks_emit: the launch failed");
    return FNN_OK;
}
