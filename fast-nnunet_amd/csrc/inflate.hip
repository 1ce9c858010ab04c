// inflate.hip - a raw deflate stream on the device that is a chain of byte-aligned segments -> its bytes, gfx950.
//
//   fnn_inflate_segments       candidates for segment starts -> the chain that covers the stream, its bytes and their CRC-32
//   fnn_inflate_segments_dyn   the same for segments that may hold dynamic-Huffman blocks: the same host code here, the
//                              kernels of inflate_dyn.hip
//   fnn_inflate_find_blocks    where a dynamic block may begin in any raw deflate stream: the kernels of inflate_any.hip
//   fnn_inflate_stream         any raw deflate stream -> its bytes and their CRC-32, speculatively from every such position:
//                              the host code here, the kernels of inflate_any.hip
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
#include "inflate_any_core.h"
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

// ---- fnn_inflate_find_blocks, fnn_inflate_stream: the host side of csrc/inflate_any.hip -------------------------------------
// The block finder's three passes over in[0, in_bytes), in_bytes > 0: mark and scan into `slices` (allocated here), the
// total back on the host in *n (the call is synchronised for it), then - `give(n)` having said where they go and how many
// fit - the positions.  The args keep what later passes need.
template <class Give> bool any_find(HipCall &c, InfAnyArgs &a, DevBuf &slices, long long *n, Give give) {
    const size_t n_slices = (size_t)((a.in_bytes + INF_ANY_SLICE - 1) / INF_ANY_SLICE);
    const size_t o_masks = 0, o_offsets = o_masks + n_slices * INF_ANY_SLICE_MASKS * 8, o_total = o_offsets + n_slices * 8,
                 o_counts = o_total + 16, total = o_counts + df_align16(n_slices * 4);
    hipError_t why;
    if (!slices.alloc(total, &why)) { c.r = why; return false; }
    a.masks = slices.as<unsigned long long>(o_masks);
    a.offsets = slices.as<long long>(o_offsets);
    a.total = slices.as<long long>(o_total);
    a.counts = slices.as<unsigned>(o_counts);
    auto pass = [&](int which, unsigned count) {
        if (!c.ok()) return;
        inf_any_launch(which, count, a, c.st);
        c.r = hipGetLastError();
    };
    pass(INF_ANY_MARK_PASS, (unsigned)n_slices);
    pass(INF_ANY_SCAN, (unsigned)n_slices);
    c.copy(n, a.total, 8, hipMemcpyDeviceToHost);
    if (!c.sync()) return false;
    if (!give(*n)) return false;
    pass(INF_ANY_WRITE, (unsigned)n_slices);
    return c.ok();
}

// what both entries refuse before any launch, beyond their own arguments
int any_check(const char *who, const void *in, int64_t in_bytes) {
    if ((uintptr_t)in % 16) return fnn_failf(FNN_E_INVALID, "%s: in must be aligned to 16 bytes", who);
    if (in_bytes > (int64_t)INT_MAX / 8 * INF_ANY_SLICE) return fnn_failf(FNN_E_UNSUPPORTED, "%s: more input than one launch addresses", who);
    return FNN_OK;
}

}  // namespace

extern "C" int fnn_inflate_find_blocks(const void *in, int64_t in_bytes, int64_t *positions, int64_t cap, int64_t *n, void *stream) {
    const char *who = "fnn_inflate_find_blocks";
    FnnOpKlog klog;
    if (!in || !n || (!positions && cap > 0)) return fnn_failf(FNN_E_INVALID, "%s: NULL argument", who);
    if (in_bytes < 0 || cap < 0) return fnn_failf(FNN_E_INVALID, "%s: negative size", who);
    if (int rc = any_check(who, in, in_bytes)) return rc;
    if (int rc = fnn_need_dev(who, {in}, "a device pointer for in")) return rc;
    if (cap > 0)
        if (int rc = fnn_need_dev(who, {positions}, "a device pointer for positions")) return rc;
    *n = 0;
    if (in_bytes == 0) return FNN_OK;
    HipCall c(stream);
    DevBuf slices;
    InfAnyArgs a{};
    a.in = (const uint8_t *)in;
    a.in_bytes = in_bytes;
    a.positions = (long long *)positions;
    a.cap = cap;
    long long total = 0;
    any_find(c, a, slices, &total, [&](long long) { return cap > 0; });
    *n = total;
    return c.finish();
}

extern "C" int fnn_inflate_stream(const void *in, int64_t in_bytes, void *out, int64_t out_bytes, uint32_t *crc32, int32_t *status,
                                  void *stream) {
    const char *who = "fnn_inflate_stream";
    FnnOpKlog klog;
    if (!in || !out || !crc32 || !status) return fnn_failf(FNN_E_INVALID, "%s: NULL argument", who);
    if (in_bytes < 0 || out_bytes < 0) return fnn_failf(FNN_E_INVALID, "%s: negative size", who);
    if (int rc = any_check(who, in, in_bytes)) return rc;
    if ((uintptr_t)out % 16) return fnn_failf(FNN_E_INVALID, "%s: out must be aligned to 16 bytes", who);
    if (int rc = fnn_need_dev(who, {in, out}, "device pointers for in and out")) return rc;
    *crc32 = 0;
    *status = FNN_INFLATE_OK;
    if (in_bytes == 0) {
        if (out_bytes != 0) *status = FNN_INFLATE_SIZE;
        return FNN_OK;
    }

    HipCall c(stream);
    DevBuf slices, per_candidate, per_member;
    InfAnyArgs a{};
    a.in = (const uint8_t *)in;
    a.in_bytes = in_bytes;
    a.out = (uint8_t *)out;
    a.out_bytes = out_bytes;
    auto pass = [&](int which, unsigned count) {
        if (!c.ok()) return;
        inf_any_launch(which, count, a, c.st);
        c.r = hipGetLastError();
    };
    long long n = 0;
    const bool found = any_find(c, a, slices, &n, [&](long long count) {
        hipError_t why;
        if (count <= 0 || count > INT_MAX) { c.r = hipErrorInvalidValue; return false; }
        if (!per_candidate.alloc((size_t)count * (8 + sizeof(InfAnyRecord)), &why)) { c.r = why; return false; }
        a.positions = per_candidate.as<long long>(0);
        a.cap = count;
        a.rec = per_candidate.as<InfAnyRecord>((size_t)count * 8);
        return true;
    });
    if (!found) return c.fail();
    std::vector<long long> positions((size_t)n);
    std::vector<InfAnyRecord> rec((size_t)n);
    pass(INF_ANY_COUNT, (unsigned)n);
    c.copy(positions.data(), a.positions, (size_t)n * 8, hipMemcpyDeviceToHost).copy(rec.data(), a.rec, (size_t)n * sizeof(InfAnyRecord), hipMemcpyDeviceToHost);
    if (!c.sync()) return c.fail();

    // the chain: from bit 0 on, a member's end is the stream's end or the next member's first bit
    std::vector<InfAnyMember> members;
    long long made_bytes = 0;
    for (size_t i = 0;;) {
        const InfAnyRecord &r = rec[i];
        if (r.reason != FNN_INFLATE_OK) { *status = r.reason; return FNN_OK; }
        if (r.reach > made_bytes) { *status = FNN_INFLATE_DISTANCE; return FNN_OK; }
        members.push_back(InfAnyMember{positions[i], made_bytes, r.end, r.len});
        made_bytes += r.len;
        if (made_bytes > out_bytes) { *status = FNN_INFLATE_SIZE; return FNN_OK; }
        if (r.end == in_bytes * 8) break;
        // (r.end > positions[i]: a member takes at least a block header, so the chain moves on and ends; r.end is a
        // candidate by the member rule - the search only finds its index)
        const auto next = std::lower_bound(positions.begin() + i + 1, positions.end(), r.end);
        if (next == positions.end() || *next != r.end) { *status = FNN_INFLATE_CHAIN; return FNN_OK; }
        i = (size_t)(next - positions.begin());
    }
    if (made_bytes != out_bytes) { *status = FNN_INFLATE_SIZE; return FNN_OK; }
    if (out_bytes == 0) return FNN_OK;

    const size_t k = members.size(), tiles = (size_t)((out_bytes + DF_CHUNK - 1) / DF_CHUNK);
    const size_t o_work = 0, o_windows = o_work + df_align16((size_t)out_bytes * 2), o_members = o_windows + (k - 1) * INF_ANY_WINDOW,
                 o_x2k = o_members + k * sizeof(InfAnyMember), o_crcs = o_x2k + sizeof(g_tables.x2k), o_made = o_crcs + df_align16(tiles * 4),
                 total = o_made + k * 4;
    if (!per_member.alloc(total)) return fnn_fail(FNN_E_HIP, "hipMalloc failed (inflate scratch)");
    a.work = per_member.as<uint16_t>(o_work);
    a.windows = per_member.as<uint8_t>(o_windows);
    a.members = per_member.as<const InfAnyMember>(o_members);
    a.x2k = per_member.as<const uint32_t>(o_x2k);
    a.crcs = per_member.as<uint32_t>(o_crcs);
    a.made = per_member.as<int>(o_made);
    std::vector<int> made(k);
    std::vector<uint32_t> crcs(tiles);
    c.copy(per_member.as<char>(o_members), members.data(), k * sizeof(InfAnyMember), hipMemcpyHostToDevice)
        .copy(per_member.as<char>(o_x2k), g_tables.x2k, sizeof(g_tables.x2k), hipMemcpyHostToDevice);
    pass(INF_ANY_EMIT, (unsigned)k);
    pass(INF_ANY_WINDOW_PASS, (unsigned)k);
    pass(INF_ANY_RESOLVE, (unsigned)k);
    c.copy(made.data(), a.made, k * 4, hipMemcpyDeviceToHost).copy(crcs.data(), a.crcs, tiles * 4, hipMemcpyDeviceToHost);
    if (!c.sync()) return c.fail();
    for (size_t i = 0; i < k; ++i)
        if (!made[i]) return fnn_failf(FNN_E_HIP, "%s: the two passes disagree on a member", who);
    uint32_t crc = 0;
    const uint32_t x_chunk = df_xpow8(DF_CHUNK, g_tables.x2k);
    for (size_t t = 0; t < tiles; ++t) {
        const long long len = t + 1 < tiles ? DF_CHUNK : out_bytes - (long long)t * DF_CHUNK;
        crc = df_crc_append(crc, crcs[t], (unsigned long long)len, g_tables.x2k, x_chunk);
    }
    *crc32 = crc;
    return FNN_OK;
}

extern "C" int fnn_inflate_segments(const void *in, int64_t in_bytes, const int64_t *starts, int64_t n_starts, void *out,
                                    int64_t out_bytes, uint32_t *crc32, int32_t *status, void *stream) {
    return inflate_run("fnn_inflate_segments", false, in, in_bytes, starts, n_starts, out, out_bytes, crc32, status, stream);
}

extern "C" int fnn_inflate_segments_dyn(const void *in, int64_t in_bytes, const int64_t *starts, int64_t n_starts, void *out,
                                        int64_t out_bytes, uint32_t *crc32, int32_t *status, void *stream) {
    return inflate_run("fnn_inflate_segments_dyn", true, in, in_bytes, starts, n_starts, out, out_bytes, crc32, status, stream);
}
