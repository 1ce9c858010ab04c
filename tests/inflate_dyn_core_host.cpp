// inflate_dyn_core_host.cpp - csrc/inflate_dyn_core.h compiled for the host (tests/test_inflate_dyn_core_host_cpu.py builds and
// runs it): the segment rule that decodes dynamic-Huffman blocks, with the tables of a block built serially in plain arrays
// (InfHostStore).
// stdin: n_starts (8 bytes, little endian), that many candidate positions (8 bytes each), then the stream to its end.
// stdout, per candidate in order: the record - end (8 bytes), len (4), reason (4) - and, for a segment that was not
// refused, the CRC-32 of its bytes (4) and the bytes.  A segment is decoded as a wave of csrc/inflate_dyn.hip does it: the image
// is filled through the sink's three calls (a match with distance < length as the periodic fill the lanes make), the
// CRC-32 taken in 64 pieces of 260 bytes and folded with deflate_core.h's arithmetic.  Every input ends with exit code 0.
#include "../fast-nnunet_amd/csrc/inflate_dyn_core.h"
#include <cstdio>
#include <cstring>
#include <vector>

static uint32_t g_tab[256];
static const DfTables g_t;

struct HostImage {
    uint8_t *img;                                                // FNN_INFLATE_SEGMENT_MAX bytes, exactly: the sanitizer sees a call outside
    void literal(int pos, unsigned v) { img[pos] = (uint8_t)v; }
    void raw(int pos, unsigned w, int k) { for (int j = 0; j < k; ++j) img[pos + j] = (uint8_t)(w >> (8 * j)); }
    void match(int pos, int len, int dist) {
        const uint8_t *src = img + pos - dist;
        for (int i = 0; i < len; ++i) img[pos + i] = src[dist >= len ? i : i % dist];
    }
};

static void put(const void *p, size_t n) { fwrite(p, 1, n, stdout); }

int main() {
    for (unsigned v = 0; v < 256; ++v) {
        uint32_t t = v;
        for (int i = 0; i < 8; ++i) t = (t >> 1) ^ ((t & 1) ? DF_POLY : 0u);
        g_tab[v] = t;
    }
    std::vector<uint8_t> all;
    for (int ch; (ch = getchar()) != EOF;) all.push_back((uint8_t)ch);
    if (all.size() < 8) return 2;
    uint64_t n = 0;
    memcpy(&n, all.data(), 8);
    if (n > (all.size() - 8) / 8) return 2;
    std::vector<long long> starts((size_t)n);
    if (n) memcpy(starts.data(), all.data() + 8, (size_t)n * 8);
    // the stream in a buffer of exactly its size, so that a read past its end is one past the allocation
    std::vector<uint8_t> stream(all.begin() + 8 + (long)n * 8, all.end());
    const long long in_bytes = (long long)stream.size();
    const uint32_t x_chunk = df_xpow8(DF_CHUNK, g_t.x2k);
    for (long long start : starts) {
        if (start < 0 || start >= in_bytes) return 2;
        std::vector<uint8_t> img(FNN_INFLATE_SEGMENT_MAX);
        HostImage sink{img.data()};
        InfHostStore store;
        const InfRecord r = inf_dyn_segment(InfBytes{stream.data(), in_bytes, start & ~3LL}, start, in_bytes, sink, store);
        const int32_t len = r.len, reason = r.reason;
        put(&r.end, 8);
        put(&len, 4);
        put(&reason, 4);
        if (reason != FNN_INFLATE_OK) continue;
        uint32_t crc = 0;
        for (int lo = 0; lo < len; lo += 260) {
            const int hi = lo + 260 < len ? lo + 260 : len;
            uint32_t c = 0xFFFFFFFFu;
            for (int p = lo; p < hi; ++p) c = g_tab[(c ^ img[p]) & 255u] ^ (c >> 8);
            crc = df_crc_append(crc, ~c, (unsigned long long)(hi - lo), g_t.x2k, x_chunk);
        }
        put(&crc, 4);
        put(img.data(), (size_t)len);
    }
    return 0;
}
