// deflate.hip - a label map on the device -> the raw-deflate bytes of its .nii.gz voxel block, gfx950.
//
//   fnn_deflate_labels       1- or 2-byte labels -> a fragment of a deflate stream, its size, and the CRC-32 of the file bytes
//   fnn_deflate_labels_dyn   the same call with per-chunk dynamic Huffman tables: this file's host code and max / scan
//                            kernels, the count and emit kernels of csrc/deflate_dyn.hip
//
// The stream format, and what a lane does with its segment of a chunk, is deflate_core.h; the steps of a wave are
// deflate_wave.h.  One wave encodes one chunk.  The rule - runs of equal elements become matches - finds what label maps
// are made of: long runs along x.
//
//   deflate_max_kernel              the maximum of a 2-byte map (a maximum below 255 is written as uint8, as the host writer does)
//   deflate_count_kernel<E, N>      a chunk -> LDS with 16-byte loads (N: every second byte of a 2-byte map), each lane
//                                   walks its segment: the bits of its tokens (kept, 2 B per segment) and its CRC-32.
//                                   The wave adds the bits up to the chunk's bytes and folds the 64 CRCs into the chunk's.
//   deflate_scan_kernel             chunk sizes -> chunk offsets in `out`, one block
//   deflate_emit_kernel<E, N>       the chunk again; a wave scan of the kept bit counts gives every lane its first bit, the
//                                   lanes OR their codes into the wave's bit buffer, which is stored by aligned vectors.
//
// LDS: segments at a pitch of 65 dwords (lane l's dword i on bank (l + i) % 32: the lanes' walks do not collide); the
// count kernel 17.5 KiB, the emit kernel 34.3 KiB.  Nothing is written outside out[0, out_bytes); no kernel keeps scratch.
#include "fnn_device.h"
#include "deflate_wave.h"
#include "deflate_dyn_launch.h"
#include "owned.h"
#include "../../include/fnn.h"
#include <climits>
#include <cstdint>
#include <vector>

namespace {

constexpr int DF_SCAN_THREADS = 1024;
constexpr int DF_MAX_THREADS = 256;

__global__ __launch_bounds__(DF_MAX_THREADS) void deflate_max_kernel(const uint16_t *in, long long n, unsigned *max_out) {
    const long long vecs = n / 8, stride = (long long)gridDim.x * DF_MAX_THREADS;
    unsigned m = 0;
    for (long long v = (long long)blockIdx.x * DF_MAX_THREADS + threadIdx.x; v < vecs; v += stride) {
        const u32x4 d = ((const u32x4 *)in)[v];
#pragma unroll
        for (int k = 0; k < 4; ++k) { m = max(m, d[k] & 0xFFFFu); m = max(m, d[k] >> 16); }
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - vecs * 8)) m = max(m, (unsigned)in[vecs * 8 + threadIdx.x]);
    for (int s = 32; s > 0; s >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, s));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(max_out, m);
}

template <int ELEM, bool NARROW>
__global__ __launch_bounds__(DF_LANES) void deflate_count_kernel(const uint8_t *in, long long n_bytes, const uint32_t *x2k,
                                                                 uint16_t *seg_bits, unsigned *chunk_bytes, uint32_t *chunk_crc) {
    __shared__ unsigned s_in[DF_LANES * DF_PITCH];
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_x2k[64];
    const int lane = threadIdx.x;
    const long long c = blockIdx.x;
    df_crc_table<DF_LANES>(s_tab, lane);
    s_x2k[lane] = x2k[lane];
    const int len = load_chunk<NARROW>(in, n_bytes, c, s_in);
    __syncthreads();
    const int mylen = df_seg_len(len, lane);
    DfCount<ELEM> cnt{s_tab};
    df_walk<ELEM>(DfBytes{s_in + lane * DF_PITCH}, mylen, cnt);
    seg_bits[c * DF_LANES + lane] = (uint16_t)cnt.bits;
    const unsigned bits = df_wave_sum(cnt.bits);
    const uint32_t crc = df_wave_crc(~cnt.crc, mylen, s_x2k, lane);
    if (lane == 0) {
        chunk_bytes[c] = df_chunk_bytes(bits);
        chunk_crc[c] = crc;
    }
}

// off[i] = the bytes of the chunks before i; off[n] = all of them
__global__ __launch_bounds__(DF_SCAN_THREADS) void deflate_scan_kernel(const unsigned *chunk_bytes, long long n, long long *off) {
    __shared__ long long s_sum[DF_SCAN_THREADS];
    const int t = threadIdx.x;
    const long long per = (n + DF_SCAN_THREADS - 1) / DF_SCAN_THREADS;
    const long long lo = min(n, t * per), hi = min(n, lo + per);
    long long sum = 0;
    for (long long i = lo; i < hi; ++i) sum += chunk_bytes[i];
    s_sum[t] = sum;
    __syncthreads();
    for (int s = 1; s < DF_SCAN_THREADS; s <<= 1) {
        const long long add = t >= s ? s_sum[t - s] : 0;
        __syncthreads();
        s_sum[t] += add;
        __syncthreads();
    }
    long long run = s_sum[t] - sum;
    for (long long i = lo; i < hi; ++i) { off[i] = run; run += chunk_bytes[i]; }
    if (t == DF_SCAN_THREADS - 1) off[n] = s_sum[t];
}

template <int ELEM, bool NARROW>
__global__ __launch_bounds__(DF_LANES) void deflate_emit_kernel(const uint8_t *in, long long n_bytes, const uint16_t *seg_bits,
                                                                const unsigned *chunk_bytes, const long long *off, uint8_t *out) {
    __shared__ unsigned s_in[DF_LANES * DF_PITCH];
    __shared__ u32x4 s_out[DF_OUT_VECS(DF_CHUNK_MAX_BYTES)];
    const int lane = threadIdx.x;
    const long long c = blockIdx.x;
    const int len = load_chunk<NARROW>(in, n_bytes, c, s_in);
    uint8_t *dst = out + off[c];
    const int mis = (int)((uintptr_t)dst & 15);                  // the chunk begins `mis` bytes into an aligned 16 bytes of `out`
    const int nbytes = (int)chunk_bytes[c];
    const int vecs = (mis + nbytes + 15) / 16;                   // <= DF_OUT_VECS(DF_CHUNK_MAX_BYTES)
    df_wave_zero(s_out, vecs, lane);
    const unsigned first_bit = df_lane_first_bit(seg_bits[c * DF_LANES + lane], lane);
    __syncthreads();
    df_wave_emit<ELEM>((unsigned *)s_out, mis, nbytes, first_bit, lane, DfBytes{s_in + lane * DF_PITCH}, df_seg_len(len, lane));
    __syncthreads();
    df_wave_store(dst, mis, nbytes, vecs, s_out, lane);
}

static const DfTables g_tables;

template <int ELEM, bool NARROW>
static void launch_pair(int pass, const uint8_t *in, long long n_bytes, long long chunks, const uint32_t *x2k, uint16_t *seg_bits,
                        unsigned *chunk_bytes, uint32_t *chunk_crc, const long long *off, uint8_t *out, hipStream_t st) {
    if (pass == 0) {
        hipLaunchKernelGGL((deflate_count_kernel<ELEM, NARROW>), dim3((unsigned)chunks), dim3(DF_LANES), 0, st, in, n_bytes, x2k,
                           seg_bits, chunk_bytes, chunk_crc);
        fnn_note_kernel("deflate_count_kernel<%d,%d>", ELEM, (int)NARROW);
    } else {
        hipLaunchKernelGGL((deflate_emit_kernel<ELEM, NARROW>), dim3((unsigned)chunks), dim3(DF_LANES), 0, st, in, n_bytes, seg_bits,
                           chunk_bytes, off, out);
        fnn_note_kernel("deflate_emit_kernel<%d,%d>", ELEM, (int)NARROW);
    }
}

}  // namespace

extern "C" int64_t fnn_deflate_bound(int64_t n_bytes) {
    if (n_bytes <= 0) return 0;
    if (n_bytes > (INT64_MAX >> 4)) return INT64_MAX;
    return (9 * n_bytes + 7) / 8 + 6 * ((n_bytes + DF_CHUNK - 1) / DF_CHUNK);
}

// fnn_deflate_labels (dyn false) and fnn_deflate_labels_dyn: one contract, one prologue, the kernels of this file or of deflate_dyn.hip
static int deflate_labels(bool dyn, const void *in, int in_elem_bytes, int64_t n_elems, int narrow_if_fits, void *out, int64_t out_cap,
                          int64_t *out_bytes, int *file_elem_bytes, uint32_t *crc32, int64_t *dynamic_chunks, void *stream) {
    FnnOpKlog klog;
    if (!in || !out || !out_bytes || !file_elem_bytes || !crc32) return fnn_fail(FNN_E_INVALID, "NULL argument");
    if (in_elem_bytes != 1 && in_elem_bytes != 2) return fnn_fail(FNN_E_INVALID, "fnn_deflate_labels: labels of 1 or 2 bytes are served");
    if (n_elems < 0) return fnn_fail(FNN_E_INVALID, "fnn_deflate_labels: negative element count");
    if ((uintptr_t)in % 16) return fnn_fail(FNN_E_INVALID, "fnn_deflate_labels: in must be aligned to 16 bytes");
    // one block per chunk: 2^31 - 1 chunks of 16 KiB
    if (n_elems > ((int64_t)INT_MAX * DF_CHUNK) / in_elem_bytes)
        return fnn_fail(FNN_E_UNSUPPORTED, "fnn_deflate_labels: too many bytes for one launch sequence");
    const long long in_bytes = (long long)n_elems * in_elem_bytes;
    if (out_cap < fnn_deflate_bound(in_bytes)) return fnn_fail(FNN_E_INVALID, "fnn_deflate_labels: out_cap is below fnn_deflate_bound");
    if (!fnn_dev_ptr(in) || !fnn_dev_ptr(out)) return fnn_fail(FNN_E_INVALID, "fnn_deflate_labels needs device pointers (no CPU path)");
    *out_bytes = 0;
    *crc32 = 0;
    *file_elem_bytes = narrow_if_fits ? 1 : in_elem_bytes;
    if (dynamic_chunks) *dynamic_chunks = 0;
    if (n_elems == 0) return FNN_OK;

    const long long max_chunks = (in_bytes + DF_CHUNK - 1) / DF_CHUNK;
    const size_t o_max = 0, o_x2k = 16, o_off = o_x2k + sizeof(g_tables.x2k), o_bytes = o_off + df_align16((size_t)(max_chunks + 1) * 8),
                 o_crc = o_bytes + df_align16((size_t)max_chunks * 4), o_bits = o_crc + df_align16((size_t)max_chunks * 4),
                 o_hdr = o_bits + df_align16((size_t)max_chunks * DF_LANES * 2), o_rec = o_hdr + (dyn ? df_align16((size_t)max_chunks * 4) : 0),
                 total = o_rec + (dyn ? (size_t)max_chunks * DF_DYN_REC_DWORDS * 4 : 0);   // (not dyn: o_hdr is the end, as it was)
    DevBuf scratch;
    if (!scratch.alloc(total)) return fnn_fail(FNN_E_HIP, "hipMalloc failed (deflate scratch)");
    unsigned *d_max = scratch.as<unsigned>(o_max);
    uint32_t *d_x2k = scratch.as<uint32_t>(o_x2k);
    long long *d_off = scratch.as<long long>(o_off);
    unsigned *d_bytes = scratch.as<unsigned>(o_bytes);
    uint32_t *d_crc = scratch.as<uint32_t>(o_crc);
    uint16_t *d_bits = scratch.as<uint16_t>(o_bits);
    uint32_t *d_hdr = scratch.as<uint32_t>(o_hdr), *d_rec = scratch.as<uint32_t>(o_rec);   // dyn only
    hipStream_t st = (hipStream_t)stream;
    hipError_t r = hipMemcpyAsync(d_x2k, g_tables.x2k, sizeof(g_tables.x2k), hipMemcpyHostToDevice, st);
    int elem = in_elem_bytes;
    if (r == hipSuccess && in_elem_bytes == 2 && narrow_if_fits) {
        unsigned h_max = 0;
        r = hipMemsetAsync(d_max, 0, 4, st);
        if (r == hipSuccess) {
            const long long want = (n_elems / 8 + DF_MAX_THREADS - 1) / DF_MAX_THREADS;
            const unsigned blocks = (unsigned)(want < 1 ? 1 : (want > 4096 ? 4096 : want));
            hipLaunchKernelGGL(deflate_max_kernel, dim3(blocks), dim3(DF_MAX_THREADS), 0, st, (const uint16_t *)in, (long long)n_elems, d_max);
            fnn_note_kernel("deflate_max_kernel");
            r = hipGetLastError();
        }
        if (r == hipSuccess) r = hipMemcpyAsync(&h_max, d_max, 4, hipMemcpyDeviceToHost, st);
        if (r == hipSuccess) r = hipStreamSynchronize(st);
        if (r == hipSuccess && h_max < 255) elem = 1;
    }
    const bool narrow = elem != in_elem_bytes;
    const uint8_t *src = (const uint8_t *)in;
    const long long n_bytes = (long long)n_elems * elem, chunks = (n_bytes + DF_CHUNK - 1) / DF_CHUNK;
    const DfDynArgs dyn_args{src, n_bytes, chunks, d_x2k, d_bits, d_bytes, d_crc, d_hdr, d_rec, d_off, (uint8_t *)out};
    for (int pass = 0; pass < 2 && r == hipSuccess; ++pass) {
        if (dyn) df_dyn_launch(pass, elem, narrow, dyn_args, st);
        else if (narrow) launch_pair<1, true>(pass, src, n_bytes, chunks, d_x2k, d_bits, d_bytes, d_crc, d_off, (uint8_t *)out, st);
        else if (elem == 1) launch_pair<1, false>(pass, src, n_bytes, chunks, d_x2k, d_bits, d_bytes, d_crc, d_off, (uint8_t *)out, st);
        else launch_pair<2, false>(pass, src, n_bytes, chunks, d_x2k, d_bits, d_bytes, d_crc, d_off, (uint8_t *)out, st);
        r = hipGetLastError();
        if (pass == 0 && r == hipSuccess) {
            hipLaunchKernelGGL(deflate_scan_kernel, dim3(1), dim3(DF_SCAN_THREADS), 0, st, d_bytes, chunks, d_off);
            fnn_note_kernel("deflate_scan_kernel");
            r = hipGetLastError();
        }
    }
    long long h_total = 0;
    std::vector<uint32_t> h_crc((size_t)chunks), h_hdr(dyn ? (size_t)chunks : 0);
    if (r == hipSuccess) r = hipMemcpyAsync(&h_total, d_off + chunks, 8, hipMemcpyDeviceToHost, st);
    if (r == hipSuccess) r = hipMemcpyAsync(h_crc.data(), d_crc, (size_t)chunks * 4, hipMemcpyDeviceToHost, st);
    if (r == hipSuccess && dyn) r = hipMemcpyAsync(h_hdr.data(), d_hdr, (size_t)chunks * 4, hipMemcpyDeviceToHost, st);
    if (r == hipSuccess) r = hipStreamSynchronize(st);
    if (r != hipSuccess) return fnn_fail(FNN_E_HIP, hipGetErrorString(r));
    uint32_t crc = 0;
    const uint32_t x_chunk = df_xpow8(DF_CHUNK, g_tables.x2k);
    for (long long c = 0; c < chunks; ++c)
        crc = df_crc_append(crc, h_crc[(size_t)c], c + 1 < chunks ? DF_CHUNK : n_bytes - c * DF_CHUNK, g_tables.x2k, x_chunk);
    *out_bytes = h_total;
    *file_elem_bytes = elem;
    *crc32 = crc;
    if (dynamic_chunks)
        for (uint32_t h : h_hdr) *dynamic_chunks += h != 0;
    return FNN_OK;
}

extern "C" int fnn_deflate_labels(const void *in, int in_elem_bytes, int64_t n_elems, int narrow_if_fits, void *out,
                                  int64_t out_cap, int64_t *out_bytes, int *file_elem_bytes, uint32_t *crc32, void *stream) {
    return deflate_labels(false, in, in_elem_bytes, n_elems, narrow_if_fits, out, out_cap, out_bytes, file_elem_bytes, crc32, nullptr, stream);
}

extern "C" int fnn_deflate_labels_dyn(const void *in, int in_elem_bytes, int64_t n_elems, int narrow_if_fits, void *out, int64_t out_cap,
                                      int64_t *out_bytes, int *file_elem_bytes, uint32_t *crc32, int64_t *dynamic_chunks, void *stream) {
    return deflate_labels(true, in, in_elem_bytes, n_elems, narrow_if_fits, out, out_cap, out_bytes, file_elem_bytes, crc32, dynamic_chunks, stream);
}
