// deflate_dyn.hip - the kernels of fnn_deflate_labels_dyn (host side: csrc/deflate.hip): a label map on the device -> the
// fragment of csrc/deflate.hip with one change - a chunk's block carries the chunk's own Huffman tables (BTYPE 10) where
// that takes fewer bits than the fixed code.  The rule is deflate_dyn_core.h; tokens, chunks, the chunk loader and the
// steps of a wave are deflate_core.h / deflate_wave.h, shared with the fixed encoder; deflate_scan_kernel is deflate.hip's.
// One wave (64 lanes) encodes one chunk.
//
//   deflate_dyn_count_kernel<E, N>  the chunk -> LDS.  Walk 1: every lane counts its segment's symbols into the chunk's
//                                   histogram (LDS atomics, the running symbol's count held in a register) and takes the
//                                   fixed code's bits and the CRC-32.  The wave builds the tables (df_dyn_tables: the sort
//                                   by all lanes; the merge of at most 285 steps, the limit and the header's run-length
//                                   pass by lane 0),
//                                   takes both totals and chooses.  Walk 2, where the tables won: the lanes' bits under
//                                   them.  Kept per chunk: bytes, CRC, the header's bit count (0: fixed code), and for the
//                                   emit pass the packed lengths and the header's bits (DF_DYN_REC_DWORDS dwords).
//   deflate_dyn_emit_kernel<E, N>   the chunk again.  Fixed code: deflate_emit_kernel's path.  Own tables: canonical codes
//                                   from the kept lengths into an LDS table (code | length << 16), the lanes OR the kept
//                                   header in, then their codes from their first bit on; lane 63 adds the end-of-block code.
//
// LDS: the count kernel 22.9 KiB (the chunk at a pitch of 65 dwords 16.3, the CRC tables 1.3, DfDynWork 5.4), the emit
// kernel 35.8 KiB (the chunk, the bit buffer 18.1, lengths and codes 1.5).  The histogram's atomics hit a handful of
// counters a few times per lane; a code lookup is one ds_read_b32 at the symbol's dword, lanes on the same symbol are one
// broadcast.  Nothing is read outside the input and the scratch of the call; nothing is written outside out[0, out_bytes);
// no kernel keeps scratch.  Every loop of the table construction has its bound next to it (deflate_dyn_core.h).
#include "fnn_device.h"
#include "deflate_wave.h"
#include "deflate_dyn_launch.h"

namespace {

struct DfWavePar {
    int l;
    __device__ __forceinline__ int lane() const { return l; }
    __device__ __forceinline__ int lanes() const { return DF_LANES; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }        // (the block is the wave)
};

template <int ELEM, bool NARROW>
__global__ __launch_bounds__(DF_LANES) void deflate_dyn_count_kernel(const uint8_t *in, long long n_bytes, const uint32_t *x2k,
                                                                     uint16_t *seg_bits, unsigned *chunk_bytes, uint32_t *chunk_crc,
                                                                     uint32_t *hdr_bits, uint32_t *rec) {
    __shared__ unsigned s_in[DF_LANES * DF_PITCH];
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_x2k[64];
    __shared__ DfDynWork k;
    const int lane = threadIdx.x;
    const long long c = blockIdx.x;
    const DfWavePar par{lane};
    df_crc_table<DF_LANES>(s_tab, lane);
    s_x2k[lane] = x2k[lane];
    for (int s = lane; s < DF_NLIT_PAD; s += DF_LANES) k.freq[s] = 0;
    const int len = load_chunk<NARROW>(in, n_bytes, c, s_in);
    __syncthreads();
    const int mylen = df_seg_len(len, lane);
    DfDynCount<ELEM> cnt{DfCount<ELEM>{s_tab}, k.freq};
    df_walk<ELEM>(DfBytes{s_in + lane * DF_PITCH}, mylen, cnt);
    cnt.finish();
    if (lane == 0) atomicAdd(&k.freq[256], 1u);
    __syncthreads();
    df_dyn_tables(k, par);
    const unsigned fixed_block = 3 + df_wave_sum(cnt.fixed.bits) + 7;
    const unsigned dyn_block = (unsigned)k.hdr_bits + df_wave_sum(df_dyn_token_bits(k, par));
    const bool dynamic = dyn_block < fixed_block;                            // the same in all lanes
    unsigned bits = cnt.fixed.bits;
    if (dynamic) {
        DfDynBits cost{k.len};
        df_walk<ELEM>(DfBytes{s_in + lane * DF_PITCH}, mylen, cost);
        bits = cost.bits;
    }
    seg_bits[c * DF_LANES + lane] = (uint16_t)bits;                          // at most 256 codes of 15 bits
    const uint32_t crc = df_wave_crc(~cnt.fixed.crc, mylen, s_x2k, lane);
    if (lane == 0) {
        chunk_bytes[c] = df_block_chunk_bytes(dynamic ? dyn_block : fixed_block);
        chunk_crc[c] = crc;
        hdr_bits[c] = dynamic ? (uint32_t)k.hdr_bits : 0u;
    }
    if (dynamic) {
        uint32_t *r = rec + c * DF_DYN_REC_DWORDS;
        for (int d = lane; d < DF_LEN_DWORDS; d += DF_LANES) r[d] = df_pack_lengths(k.len, d);
        for (int d = lane; d < DF_HDR_DWORDS; d += DF_LANES) r[DF_LEN_DWORDS + d] = k.hdr[d];
    }
}

template <int ELEM, bool NARROW>
__global__ __launch_bounds__(DF_LANES) void deflate_dyn_emit_kernel(const uint8_t *in, long long n_bytes, const uint16_t *seg_bits,
                                                                    const unsigned *chunk_bytes, const uint32_t *hdr_bits,
                                                                    const uint32_t *rec, const long long *off, uint8_t *out) {
    __shared__ unsigned s_in[DF_LANES * DF_PITCH];
    __shared__ u32x4 s_out[DF_OUT_VECS(DF_CHUNK_MAX_BYTES)];
    __shared__ uint32_t s_code[DF_NLIT_PAD];
    __shared__ uint32_t s_next[16];
    __shared__ uint8_t s_len[DF_NLIT_PAD];
    const int lane = threadIdx.x;
    const long long c = blockIdx.x;
    const int len = load_chunk<NARROW>(in, n_bytes, c, s_in);
    uint8_t *dst = out + off[c];
    const int mis = (int)((uintptr_t)dst & 15);                  // the chunk begins `mis` bytes into an aligned 16 bytes of `out`
    const int nbytes = (int)chunk_bytes[c];                      // <= the fixed code's: the choice
    const int vecs = (mis + nbytes + 15) / 16;                   // <= DF_OUT_VECS(DF_CHUNK_MAX_BYTES)
    const int hb = (int)hdr_bits[c];
    const unsigned bits = seg_bits[c * DF_LANES + lane];
    unsigned *buf = (unsigned *)s_out;
    df_wave_zero(s_out, vecs, lane);
    if (hb == 0) {
        const unsigned first_bit = df_lane_first_bit(bits, lane);
        __syncthreads();
        df_wave_emit<ELEM>(buf, mis, nbytes, first_bit, lane, DfBytes{s_in + lane * DF_PITCH}, df_seg_len(len, lane));
    } else {
        const uint32_t *r = rec + c * DF_DYN_REC_DWORDS;
        for (int d = lane; d < DF_LEN_DWORDS; d += DF_LANES) {
            const uint32_t v = r[d];
#pragma unroll
            for (int i = 0; i < 8; ++i) s_len[d * 8 + i] = (uint8_t)((v >> (4 * i)) & 15u);
        }
        const unsigned first_bit = (unsigned)hb + df_lane_bits_before(bits, lane);
        __syncthreads();
        df_canonical(s_len, DF_NLIT, s_code, s_next, DfWavePar{lane});
        for (int d = lane; d * 32 < hb; d += DF_LANES) {         // the header: dword d lies 32 d bits behind the chunk's first
            const uint32_t v = r[DF_LEN_DWORDS + d];
            const int w = mis / 4 + d, sh = (mis & 3) * 8;
            atomicOr(buf + w, v << sh);
            if (sh) atomicOr(buf + w + 1, v >> (32 - sh));       // (behind the header lie 32 bits of the chunk or more)
        }
        DfDynEmit<ELEM> em{DfEmit<ELEM>(buf, (unsigned)mis * 8 + first_bit), s_code};
        df_walk<ELEM>(DfBytes{s_in + lane * DF_PITCH}, df_seg_len(len, lane), em);
        if (lane == DF_LANES - 1) em.symbol(256);                // its bits end where the tokens end
        em.em.finish();
        // the stored block's header, its padding and its LEN are zeros, which the buffer holds; NLEN = FF FF
        if (lane < 2) {
            const int b = mis + nbytes - 2 + lane;
            atomicOr(buf + (b >> 2), 0xFFu << ((b & 3) * 8));
        }
    }
    __syncthreads();
    df_wave_store(dst, mis, nbytes, vecs, s_out, lane);
}

template <int ELEM, bool NARROW> void launch_pair(int pass, const DfDynArgs &a, hipStream_t st) {
    if (pass == 0) {
        hipLaunchKernelGGL((deflate_dyn_count_kernel<ELEM, NARROW>), dim3((unsigned)a.chunks), dim3(DF_LANES), 0, st, a.in, a.n_bytes,
                           a.x2k, a.seg_bits, a.chunk_bytes, a.chunk_crc, a.hdr_bits, a.rec);
        fnn_note_kernel("deflate_dyn_count_kernel<%d,%d>", ELEM, (int)NARROW);
    } else {
        hipLaunchKernelGGL((deflate_dyn_emit_kernel<ELEM, NARROW>), dim3((unsigned)a.chunks), dim3(DF_LANES), 0, st, a.in, a.n_bytes,
                           a.seg_bits, a.chunk_bytes, a.hdr_bits, a.rec, a.off, a.out);
        fnn_note_kernel("deflate_dyn_emit_kernel<%d,%d>", ELEM, (int)NARROW);
    }
}

}  // namespace

void df_dyn_launch(int pass, int elem, bool narrow, const DfDynArgs &a, hipStream_t st) {
    if (narrow) launch_pair<1, true>(pass, a, st);
    else if (elem == 1) launch_pair<1, false>(pass, a, st);
    else launch_pair<2, false>(pass, a, st);
}
