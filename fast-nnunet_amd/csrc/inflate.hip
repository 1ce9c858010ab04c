// inflate.hip - a raw deflate stream on the device that is a chain of byte-aligned segments -> its bytes, gfx950.
//
//   fnn_inflate_segments       candidates for segment starts -> the chain that covers the stream, its bytes and their CRC-32
//   fnn_inflate_segments_dyn   the same for segments that may hold dynamic-Huffman blocks: the same host code here, the
//                              kernels of inflate_dyn.hip
//
// The segment rule, and the decode step all passes share, is inflate_core.h; what the kernels of both files share - the
// register window, the LDS image, the CRC and the store of a finished image - is inflate_wave.h.  One wave decodes one segment; the token loop
// is serial and wave-uniform - its bit reader, positions and branches live in scalar registers - and the 64 lanes share
// the bytes of a token.
//
//   inflate_count_kernel   one wave per candidate: decodes without keeping a byte (a match is judged by its distance and
//                          the position alone) and records the segment's end, size and reason.  No LDS.
//   inflate_emit_kernel    one wave per chain member: decodes into the wave's 16 KiB LDS image of the segment - a literal
//                          is one lane's store, a match goes in strides of 64 lanes and reads the image back (distance <
//                          length: byte i comes from i modulo the distance, a periodic fill) - then takes the CRC-32 of
//                          the image, 260 bytes per lane (65 dwords: lane l's dword i lies on bank (l + i) % 32), and
//                          stores the image at the member's offset in `out` by aligned 16-byte vectors, the ends singly.
//
// The compressed bytes reach the decoder through a register window: lane l holds dword l of 256 stream bytes, loaded with
// one coalesced aligned load, and the reader takes dword after dword out of it with v_readlane; the next window is loaded
// when the current one is entered, 64 dwords before it is needed.  Bytes past in_bytes are never loaded: they read as 0.
//
// The chain is followed on the host between the two passes (as fnn_deflate_labels folds its CRCs there).  Nothing is read
// outside in[0, in_bytes) or written outside out[0, out_bytes); no kernel keeps scratch.
#include "host_call.h"
#include "inflate_wave.h"
#include <algorithm>
#include <climits>
#include <cstdint>
#include <vector>

namespace {

__global__ __launch_bounds__(DF_LANES) void inflate_count_kernel(const uint8_t *in, long long in_bytes, const long long *starts,
                                                                InfRecord *rec) {
    const int lane = threadIdx.x;
    const long long start = starts[blockIdx.x];
    InfNoSink sink;
    const InfRecord r = inf_segment(InfWindow(in, in_bytes, start, lane), start, in_bytes, sink);
    if (lane == 0) rec[blockIdx.x] = r;
}

__global__ __launch_bounds__(DF_LANES) void inflate_emit_kernel(const uint8_t *in, long long in_bytes, const InfMember *members,
                                                               const uint32_t *x2k, uint8_t *out, InfMade *made) {
    __shared__ u32x4 s_img[DF_OUT_VECS(FNN_INFLATE_SEGMENT_MAX)];
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_x2k[64];
    const int lane = threadIdx.x;
    const InfMember m = members[blockIdx.x];
    df_crc_table<DF_LANES>(s_tab, lane);
    s_x2k[lane] = x2k[lane];
    uint8_t *dst = out + m.off;
    const int mis = (int)((uintptr_t)dst & 15);                  // the segment begins `mis` bytes into an aligned 16 bytes of `out`
    InfImage sink{(uint8_t *)s_img + mis, lane};
    const InfRecord r = inf_segment(InfWindow(in, in_bytes, m.start, lane), m.start, in_bytes, sink);
    __syncthreads();
    if (r.reason != FNN_INFLATE_OK) {
        if (lane == 0) made[blockIdx.x] = InfMade{0u, -1};
        return;
    }
    inf_wave_finish(dst, mis, r.len, s_img, s_tab, s_x2k, made, lane);
}

static const DfTables g_tables;

// the host side of both entries; `dyn`: the kernels of csrc/inflate_dyn.hip, which decode dynamic-Huffman blocks too
int inflate_run(const char *who, bool dyn, const void *in, int64_t in_bytes, const int64_t *starts, int64_t n_starts, void *out,
                int64_t out_bytes, uint32_t *crc32, int32_t *status, void *stream) {
    FnnOpKlog klog;
    if (!in || !starts || !out || !crc32 || !status) return fnn_failf(FNN_E_INVALID, "%s: NULL argument", who);
    if (in_bytes < 0 || n_starts < 0 || out_bytes < 0) return fnn_failf(FNN_E_INVALID, "%s: negative size", who);
    if ((uintptr_t)in % 16) return fnn_failf(FNN_E_INVALID, "%s: in must be aligned to 16 bytes", who);
    if ((uintptr_t)out % 16) return fnn_failf(FNN_E_INVALID, "%s: out must be aligned to 16 bytes", who);
    if (n_starts > 0 && starts[0] != 0) return fnn_failf(FNN_E_INVALID, "%s: starts must begin at 0", who);
    for (int64_t i = 1; i < n_starts; ++i)
        if (starts[i] <= starts[i - 1]) return fnn_failf(FNN_E_INVALID, "%s: starts must be strictly ascending", who);
    if (n_starts > 0 && starts[n_starts - 1] >= in_bytes) return fnn_failf(FNN_E_INVALID, "%s: every start must lie below in_bytes", who);
    if (n_starts > INT_MAX) return fnn_failf(FNN_E_UNSUPPORTED, "%s: more candidates than one launch addresses", who);
    if (int rc = fnn_need_dev(who, {in, out}, "device pointers for in and out")) return rc;
    *crc32 = 0;
    *status = FNN_INFLATE_OK;
    if (n_starts == 0 || in_bytes == 0) {
        if (out_bytes != 0) *status = FNN_INFLATE_SIZE;
        return FNN_OK;
    }

    const size_t n = (size_t)n_starts;
    const size_t o_starts = 0, o_rec = o_starts + df_align16(n * 8), o_mem = o_rec + n * sizeof(InfRecord),
                 o_made = o_mem + n * sizeof(InfMember), o_x2k = o_made + df_align16(n * sizeof(InfMade)),
                 total = o_x2k + sizeof(g_tables.x2k);
    DevBuf scratch;
    if (!scratch.alloc(total)) return fnn_fail(FNN_E_HIP, "hipMalloc failed (inflate scratch)");
    HipCall c(stream);
    std::vector<InfRecord> rec(n);
    const InfDynArgs args{(const uint8_t *)in, (long long)in_bytes, scratch.as<const long long>(o_starts), scratch.as<InfRecord>(o_rec),
                          scratch.as<const InfMember>(o_mem), scratch.as<const uint32_t>(o_x2k), (uint8_t *)out, scratch.as<InfMade>(o_made)};
    c.copy(scratch.as<char>(o_starts), starts, n * 8, hipMemcpyHostToDevice);
    if (dyn) {
        if (c.ok()) {
            inf_dyn_launch(0, (unsigned)n, args, c.st);
            c.r = hipGetLastError();
        }
    } else {
        c.launch(inflate_count_kernel, dim3((unsigned)n), dim3(DF_LANES), 0, args.in, args.in_bytes, args.starts, args.rec);
        fnn_note_kernel("inflate_count_kernel");
    }
    c.copy(rec.data(), scratch.as<char>(o_rec), n * sizeof(InfRecord), hipMemcpyDeviceToHost);
    if (!c.sync()) return c.fail();

    // the chain: from candidate 0 on, a member's end is the input's end or the next member's start
    std::vector<InfMember> members;
    long long made_bytes = 0;
    for (size_t i = 0;;) {
        const InfRecord &r = rec[i];
        if (r.reason != FNN_INFLATE_OK) { *status = r.reason; return FNN_OK; }
        members.push_back(InfMember{(long long)starts[i], made_bytes});
        made_bytes += r.len;
        if (made_bytes > out_bytes) { *status = FNN_INFLATE_SIZE; return FNN_OK; }
        if (r.end == in_bytes) break;
        // (r.end > starts[i]: a segment takes at least its empty stored block, so the chain moves on and ends)
        const int64_t *next = std::lower_bound(starts + i + 1, starts + n, (int64_t)r.end);
        if (next == starts + n || *next != r.end) { *status = FNN_INFLATE_CHAIN; return FNN_OK; }
        i = (size_t)(next - starts);
    }
    if (made_bytes != out_bytes) { *status = FNN_INFLATE_SIZE; return FNN_OK; }

    const size_t k = members.size();
    std::vector<InfMade> made(k);
    c.copy(scratch.as<char>(o_mem), members.data(), k * sizeof(InfMember), hipMemcpyHostToDevice)
        .copy(scratch.as<char>(o_x2k), g_tables.x2k, sizeof(g_tables.x2k), hipMemcpyHostToDevice);
    if (dyn) {
        if (c.ok()) {
            inf_dyn_launch(1, (unsigned)k, args, c.st);
            c.r = hipGetLastError();
        }
    } else {
        c.launch(inflate_emit_kernel, dim3((unsigned)k), dim3(DF_LANES), 0, args.in, args.in_bytes, args.members, args.x2k, args.out, args.made);
        fnn_note_kernel("inflate_emit_kernel");
    }
    c.copy(made.data(), scratch.as<char>(o_made), k * sizeof(InfMade), hipMemcpyDeviceToHost);
    if (!c.sync()) return c.fail();
    uint32_t crc = 0;
    const uint32_t x_chunk = df_xpow8(DF_CHUNK, g_tables.x2k);
    for (size_t i = 0; i < k; ++i) {
        if (made[i].len != (i + 1 < k ? members[i + 1].off : made_bytes) - members[i].off) return fnn_failf(FNN_E_HIP, "%s: the two passes disagree on a segment", who);
        crc = df_crc_append(crc, made[i].crc, (unsigned long long)made[i].len, g_tables.x2k, x_chunk);
    }
    *crc32 = crc;
    return FNN_OK;
}

}  // namespace

extern "C" int fnn_inflate_segments(const void *in, int64_t in_bytes, const int64_t *starts, int64_t n_starts, void *out,
                                    int64_t out_bytes, uint32_t *crc32, int32_t *status, void *stream) {
    return inflate_run("fnn_inflate_segments", false, in, in_bytes, starts, n_starts, out, out_bytes, crc32, status, stream);
}

extern "C" int fnn_inflate_segments_dyn(const void *in, int64_t in_bytes, const int64_t *starts, int64_t n_starts, void *out,
                                        int64_t out_bytes, uint32_t *crc32, int32_t *status, void *stream) {
    return inflate_run("fnn_inflate_segments_dyn", true, in, in_bytes, starts, n_starts, out, out_bytes, crc32, status, stream);
}
