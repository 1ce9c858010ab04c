// inflate_any_core_host.cpp - csrc/inflate_any_core.h compiled for the host (tests/test_inflate_any_core_host_cpu.py builds and
// runs it): the block finder, the member rule, the chain, the 16-bit entries with their markers, the windows and the resolved
// bytes, done pass by pass as fnn_inflate_stream does them, with the tables of a block built serially (InfHostStore).
// stdin: out_bytes (8 bytes, little endian), then the stream to its end.
// stdout: the number of candidates (8) and their bit positions (8 each); per candidate its record - end (8), len (8),
// reason (4), reach (4); the status (4).  For status 0 then: the number of members (8); per member start, off, len (8 each)
// and its len entries (2 each); the windows (32768 each, one per member but the last); the out_bytes final bytes and their
// CRC-32 (4).
// The passes mirror csrc/inflate_any.hip: every bit position is put to inf_any_maybe first and, whatever that says, to the
// full rule - a candidate that the first test would have dropped is exit code 3; a member's entries go through a ring of
// 32768 slots addressed by the absolute output position, a match in rounds of 64 lanes that all read before any writes,
// and are kept in a buffer of exactly the member's length, so that the sanitizer sees a write outside it; the CRC-32 is
// taken in pieces of 256 bytes, folded per 16 KiB and then along the output.  Every input ends with exit code 0.
#include "../fast-nnunet_amd/csrc/inflate_any_core.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

static uint32_t g_tab[256];
static const DfTables g_t;

static void put(const void *p, size_t n) { fwrite(p, 1, n, stdout); }
template <class T> static void put_as(long long v) { const T t = (T)v; put(&t, sizeof t); }

struct Known {
    const std::vector<long long> &pos;
    bool operator()(long long bit) const {
        const auto it = std::lower_bound(pos.begin(), pos.end(), bit);
        return it != pos.end() && *it == bit;
    }
};
struct EndsAt {
    long long end;
    bool operator()(long long bit) const { return bit == end; }
};

struct HostRing {
    std::vector<uint16_t> ring = std::vector<uint16_t>(INF_ANY_WINDOW);
    uint16_t *kept;                                              // exactly the member's entries
    long long off;
    unsigned slot(long long pos) const { return (unsigned)(off + pos) & (INF_ANY_WINDOW - 1); }
    void set(long long pos, unsigned e) { ring[slot(pos)] = kept[pos] = (uint16_t)e; }
    void literal(long long pos, unsigned v) { set(pos, v); }
    void raw(long long pos, unsigned w, int k) { for (int j = 0; j < k; ++j) set(pos + j, (w >> (8 * j)) & 255u); }
    void match(long long pos, int len, int dist) {
        for (int round = 0; round < len; round += 64) {
            unsigned e[64];
            const int n = len - round < 64 ? len - round : 64;
            for (int l = 0; l < n; ++l) {
                const int i = round + l;
                const long long src = pos - dist + (dist >= len ? i : i % dist);
                e[l] = inf_any_entry(src, src < 0 ? 0u : ring[slot(src)]);
            }
            for (int l = 0; l < n; ++l) set(pos + round + l, e[l]);
        }
    }
};

static InfBytes reader(const std::vector<uint8_t> &s, long long bit) { return InfBytes{s.data(), (long long)s.size(), (bit >> 5) * 4}; }

int main() {
    for (unsigned v = 0; v < 256; ++v) {
        uint32_t t = v;
        for (int i = 0; i < 8; ++i) t = (t >> 1) ^ ((t & 1) ? DF_POLY : 0u);
        g_tab[v] = t;
    }
    std::vector<uint8_t> all;
    for (int ch; (ch = getchar()) != EOF;) all.push_back((uint8_t)ch);
    if (all.size() < 8) return 2;
    long long out_bytes = 0;
    memcpy(&out_bytes, all.data(), 8);
    if (out_bytes < 0 || out_bytes > (1 << 28)) return 2;
    // the stream in a buffer of exactly its size, so that a read past its end is one past the allocation
    const std::vector<uint8_t> stream(all.begin() + 8, all.end());
    const long long in_bytes = (long long)stream.size();

    // find
    std::vector<long long> pos;
    InfHostStore store;
    for (long long p = 0; p < in_bytes * 8; ++p) {
        unsigned w[4];
        InfBytes rd = reader(stream, p);
        for (unsigned &d : w) d = rd.next();
        const int sh = (int)(p & 31);
        const unsigned long long lo = w[0] | (unsigned long long)w[1] << 32, hi = w[2] | (unsigned long long)w[3] << 32;
        const bool may = inf_any_maybe(sh ? lo >> sh | hi << (64 - sh) : lo, (unsigned)(hi >> sh));
        if (inf_any_candidate(reader(stream, p), p, in_bytes, store)) {
            if (p && !may) return 3;
            pos.push_back(p);
        }
    }
    put_as<long long>((long long)pos.size());
    if (!pos.empty()) put(pos.data(), pos.size() * 8);

    // count
    std::vector<InfAnyRecord> rec;
    Known known{pos};
    for (long long p : pos) {
        InfAnyNoSink none;
        const InfAnyRecord r = inf_any_member(reader(stream, p), p, in_bytes, out_bytes, none, store, known);
        rec.push_back(r);
        put_as<long long>(r.end);
        put_as<long long>(r.len);
        put_as<int32_t>(r.reason);
        put_as<int32_t>(r.reach);
    }

    // chain
    struct Member { long long start, off, end, len; };
    std::vector<Member> members;
    int status = FNN_INFLATE_OK;
    long long made = 0;
    if (in_bytes == 0) status = out_bytes ? FNN_INFLATE_SIZE : FNN_INFLATE_OK;
    for (size_t i = 0; in_bytes > 0;) {
        const InfAnyRecord &r = rec[i];
        if (r.reason != FNN_INFLATE_OK) { status = r.reason; break; }
        if (r.reach > made) { status = FNN_INFLATE_DISTANCE; break; }
        members.push_back(Member{pos[i], made, r.end, r.len});
        made += r.len;
        if (made > out_bytes) { status = FNN_INFLATE_SIZE; break; }
        if (r.end == in_bytes * 8) break;
        const auto next = std::lower_bound(pos.begin() + i + 1, pos.end(), r.end);
        if (next == pos.end() || *next != r.end) { status = FNN_INFLATE_CHAIN; break; }
        i = (size_t)(next - pos.begin());
    }
    if (status == FNN_INFLATE_OK && made != out_bytes) status = FNN_INFLATE_SIZE;
    put_as<int32_t>(status);
    if (status != FNN_INFLATE_OK) return 0;

    // emit
    const size_t k = members.size();
    put_as<long long>((long long)k);
    std::vector<std::vector<uint16_t>> entries(k);
    for (size_t m = 0; m < k; ++m) {
        entries[m].resize((size_t)members[m].len);
        HostRing ring;
        ring.kept = entries[m].data();
        ring.off = members[m].off;
        EndsAt ends{members[m].end};
        const InfAnyRecord r = inf_any_member(reader(stream, members[m].start), members[m].start, in_bytes, members[m].len, ring, store, ends);
        if (r.reason != FNN_INFLATE_OK || r.len != members[m].len || r.end != members[m].end) return 4;
        put_as<long long>(members[m].start);
        put_as<long long>(members[m].off);
        put_as<long long>(members[m].len);
        if (r.len) put(entries[m].data(), (size_t)r.len * 2);
    }

    // windows, as the window kernel makes them
    std::vector<std::vector<uint8_t>> windows(k ? k - 1 : 0, std::vector<uint8_t>(INF_ANY_WINDOW));
    for (size_t m = 0; m + 1 < k; ++m) {
        const long long len = members[m].len;
        for (int j = 0; j < INF_ANY_WINDOW; ++j) {
            const long long at = len - INF_ANY_WINDOW + j;       // a position of the member, or before it
            unsigned v = 0;
            if (at >= 0) {
                const unsigned e = entries[m][(size_t)at];
                v = e & INF_ANY_MARK ? (m ? windows[m - 1][e & (INF_ANY_WINDOW - 1)] : 0u) : e;
            } else if (m) {
                v = windows[m - 1][(size_t)(j + len)];
            }
            windows[m][j] = (uint8_t)v;
        }
        put(windows[m].data(), INF_ANY_WINDOW);
    }

    // resolve
    std::vector<uint8_t> out((size_t)out_bytes);
    for (size_t m = 0; m < k; ++m)
        for (long long i = 0; i < members[m].len; ++i) {
            const unsigned e = entries[m][(size_t)i];
            out[(size_t)(members[m].off + i)] = (uint8_t)(e & INF_ANY_MARK ? (m ? windows[m - 1][e & (INF_ANY_WINDOW - 1)] : 0u) : e);
        }
    uint32_t crc = 0;
    const uint32_t x_chunk = df_xpow8(DF_CHUNK, g_t.x2k);
    for (long long t0 = 0; t0 < out_bytes; t0 += DF_CHUNK) {
        const long long t1 = t0 + DF_CHUNK < out_bytes ? t0 + DF_CHUNK : out_bytes;
        uint32_t tile = 0;
        for (long long lo = t0; lo < t1; lo += DF_SEG) {
            const long long hi = lo + DF_SEG < t1 ? lo + DF_SEG : t1;
            uint32_t c = 0xFFFFFFFFu;
            for (long long p = lo; p < hi; ++p) c = g_tab[(c ^ out[(size_t)p]) & 255u] ^ (c >> 8);
            tile = lo == t0 ? ~c : df_mulmod(tile, df_xpow8((unsigned long long)(hi - lo), g_t.x2k)) ^ ~c;
        }
        crc = df_crc_append(crc, tile, (unsigned long long)(t1 - t0), g_t.x2k, x_chunk);
    }
    if (out_bytes) put(out.data(), (size_t)out_bytes);
    put_as<uint32_t>(crc);
    return 0;
}
