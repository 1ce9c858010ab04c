// inflate_dyn.hip - the kernels of fnn_inflate_segments_dyn (its host code is csrc/inflate.hip's): segments that may hold
// dynamic-Huffman blocks, gfx950.  The rule is inflate_dyn_core.h; the window, the image, the CRC and the store are
// inflate_wave.h's, as in the fixed route.
//
//   inflate_dyn_count_kernel   one wave per candidate: decodes without keeping a byte and records end, size and reason
//   inflate_dyn_emit_kernel    one wave per chain member: decodes into the wave's LDS image, then CRC and store
//
// The token loop is serial and wave-uniform, as in inflate.hip.  What is new is a block's tables (InfWaveStore), built by
// the 64 lanes and decoded canonically across them (InfWaveStore, inflate_dyn_wave.h) - no lookup table is filled:
//   * the block's code lengths lie in LDS, one 16-bit entry each (s_seq);
//   * count: lane j looks at symbols j, 64 + j, ... (at most 5 of the 286); per length l a ballot says which lanes hold a
//     symbol of that length, lane l adds the ballot's population to its count, and a lane whose symbol has length l takes
//     its rank among them - the count before, plus the lanes below it in the ballot - and leaves it next to the length;
//   * the rule (inf_build_code) reads the 15 counts with v_readlane, makes the Kraft check and hands lane l the first
//     code of length l, left-justified to 15 bits, the left-justified limit behind its last code, and the place of its
//     first symbol in the sorted list;
//   * sort: every lane stores its symbols at place[length] + rank in the list (s_sorted), sorted by (length, symbol);
//   * symbol: the 15 peeked bits, reversed, are compared by lanes 1 .. 15 with their limits; the lowest lane of the
//     ballot is the code's length l, lane l's first code and place come by v_readlane, and one LDS read of the list gives
//     the symbol.  No lane in the ballot: the pattern belongs to no symbol (an accepted incomplete set).
// All three codes of a block - the code-length code, literal / length, distance - go the same way.  Every index formed
// from stream bits is bounded where it is used - clamped to the 288 entries of the literal / length list, masked to the 32
// of the other two; positions in s_seq are bounded by the rule (a run is checked against HLIT + HDIST before it is stored).
//
// LDS: the tables take 704 B (s_seq) + 704 B (the three lists) = 1408 B.  The count kernel has nothing else.  In the emit
// kernel they share their place with the CRC table and the field's powers (1280 B), which are made only when the decode is
// over: 16 400 + 1408 = 17 808 B against the fixed emit kernel's 17 680 B - 9 workgroups per CU by the 160 KiB of LDS, as
// the fixed kernel has.  No kernel keeps scratch: nothing per lane is indexed by a runtime value.
#include "fnn_device.h"
#include "inflate_dyn_wave.h"

namespace {

__global__ __launch_bounds__(DF_LANES) void inflate_dyn_count_kernel(const uint8_t *in, long long in_bytes, const long long *starts,
                                                                    InfRecord *rec) {
    __shared__ uint16_t s_tables[INF_TABLE_BYTES / 2];
    const int lane = threadIdx.x;
    const long long start = starts[blockIdx.x];
    InfNoSink sink;
    InfWaveStore store(s_tables, lane);
    const InfRecord r = inf_dyn_segment(InfWindow(in, in_bytes, start, lane), start, in_bytes, sink, store);
    if (lane == 0) rec[blockIdx.x] = r;
}

__global__ __launch_bounds__(DF_LANES) void inflate_dyn_emit_kernel(const uint8_t *in, long long in_bytes, const InfMember *members,
                                                                   const uint32_t *x2k, uint8_t *out, InfMade *made) {
    __shared__ u32x4 s_img[DF_OUT_VECS(FNN_INFLATE_SEGMENT_MAX)];
    // the block's tables while the segment is decoded, then the CRC's byte table (256 dwords) and the field's powers (64)
    __shared__ uint32_t s_small[INF_TABLE_BYTES / 4];
    static_assert(INF_TABLE_BYTES >= (256 + 64) * 4, "the CRC's tables fit where the block's were");
    const int lane = threadIdx.x;
    const InfMember m = members[blockIdx.x];
    uint8_t *dst = out + m.off;
    const int mis = (int)((uintptr_t)dst & 15);                  // the segment begins `mis` bytes into an aligned 16 bytes of `out`
    InfImage sink{(uint8_t *)s_img + mis, lane};
    InfWaveStore store((uint16_t *)s_small, lane);
    const InfRecord r = inf_dyn_segment(InfWindow(in, in_bytes, m.start, lane), m.start, in_bytes, sink, store);
    __syncthreads();
    if (r.reason != FNN_INFLATE_OK) {
        if (lane == 0) made[blockIdx.x] = InfMade{0u, -1};
        return;
    }
    uint32_t *s_tab = s_small, *s_x2k = s_small + 256;
    df_crc_table<DF_LANES>(s_tab, lane);
    s_x2k[lane] = x2k[lane];
    __syncthreads();
    inf_wave_finish(dst, mis, r.len, s_img, s_tab, s_x2k, made, lane);
}

}  // namespace

void inf_dyn_launch(int pass, unsigned n, const InfDynArgs &a, hipStream_t st) {
    if (pass == 0) {
        hipLaunchKernelGGL(inflate_dyn_count_kernel, dim3(n), dim3(DF_LANES), 0, st, a.in, a.in_bytes, a.starts, a.rec);
        fnn_note_kernel("inflate_dyn_count_kernel");
    } else {
        hipLaunchKernelGGL(inflate_dyn_emit_kernel, dim3(n), dim3(DF_LANES), 0, st, a.in, a.in_bytes, a.members, a.x2k, a.out, a.made);
        fnn_note_kernel("inflate_dyn_emit_kernel");
    }
}
