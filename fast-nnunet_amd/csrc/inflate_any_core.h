// inflate_any_core.h - a raw deflate stream (RFC 1951) that nobody cut into segments, as a speculative decoder sees it.  Host
// and device from the same text (tests/inflate_any_core_host.cpp compiles it for the host); the kernels around it are
// csrc/inflate_any.hip, tests/inflate_any_ref.py restates the rule in Python and the tests compare record for record.
//
// Stream: in[0, in_bytes) inflates to exactly out_bytes bytes.
//
// Candidate: a bit position p at which a decode may begin.  Bit 0 is one.  Any other p is one where
//   * the three bits at p are BFINAL 0, BTYPE 10 (the value 4, first bit lowest),
//   * the table header behind them passes checks 1 - 5 of inflate_dyn_core.h, made by that header's InfDynCodes::header in
//     its order - the accepted set is exactly zlib's -
//   * and the header ends at or before the input's end (header()'s limit is the input's end).
// inf_any_maybe() is a cheap necessary condition on the first 74 bits (the three bits, HLIT <= 286, HDIST <= 30, the
// code-length code's Kraft sum exactly 1): what it lets through is checked in full, so it does not change the set.
//
// Member: the decode from a candidate, with bit granularity: block after block - stored, fixed and dynamic ones where they
// occur - until a non-final block ends at a bit position that is itself a candidate (`is_cand`), which is the next
// member's start, or until a BFINAL block ends.  That is the stream's end where the block's last byte is the input's last
// (the record's end is then 8 * in_bytes); where bytes follow it is FNN_INFLATE_FINAL.  BTYPE 3 and every refusal of the
// rules before keep their reasons; a member that runs out of input is FNN_INFLATE_END.  There is no limit of
// FNN_INFLATE_SEGMENT_MAX and no input budget: the length is counted in 64 bits and a token that would pass out_bytes is
// FNN_INFLATE_OUTPUT.  A match may reach back before the member's own first byte (by at most 32768, the format's longest
// distance): the member records the furthest it does (`reach`), and the chain, which knows the member's output offset,
// refuses reach > offset with FNN_INFLATE_DISTANCE.
//
// Loops: the limit - the input's end - is compared with used() behind everything an iteration of the block loop or the
// token loop drops, and for a stored block before its first byte.  An iteration drops at least 3 bits (a block header),
// 1 (a token) or 8 (a stored unit of up to 4 bytes), so at most 8 * in_bytes + 1 iterations run whatever the input holds,
// none of them past the limit by more than one token: the reader is asked for at most three dwords beyond the input, which
// it answers with zeros.
//
// Markers: the sink is handed 64-bit positions, and match() a distance that may exceed the position.  The emit pass writes
// 16-bit entries: a literal or stored byte as 0 .. 255; a match source inside the member copies the entry as it is, marker
// or not; a source before the member's first byte writes 0x8000 | (32768 + pos - dist), an index into the 32768 resolved
// bytes that precede the member (its window).  inf_any_entry() is that rule for one entry.
#pragma once
#include "inflate_dyn_core.h"

constexpr int INF_ANY_WINDOW = 32768;                    // the furthest a match reaches back, and the bytes of a window
constexpr unsigned INF_ANY_MARK = 0x8000u;

// what the decode of one candidate leaves: `end` the bit behind the member in the stream (8 * in_bytes: the stream's end;
// -1 when it was refused), `len` the output bytes made (until the refusal), `reason`, and how far before its own first byte
// the member reaches at the most (0 .. 32768)
struct InfAnyRecord {
    long long end;
    long long len;
    int reason;
    int reach;
};

// The first 96 bits at a bit position (lo: bits 0 .. 63, hi: 64 .. 95) -> whether a candidate may begin there.
DF_HD bool inf_any_maybe(unsigned long long lo, unsigned hi) {
    if ((lo & 7u) != 4u) return false;
    if (((lo >> 3) & 31u) > 29u || ((lo >> 8) & 31u) > 29u) return false;
    const int hclen = 4 + (int)((lo >> 13) & 15u);
    // the 3-bit lengths from bit 17 on: 15 of them in lo's bits 17 .. 61, the others from bit 62 on
    const unsigned long long rest = lo >> 62 | (unsigned long long)hi << 2;
    int kraft = 0;                                       // in units of 2^-7
    for (int i = 0; i < 19; ++i) {
        const int len = (int)((i < 15 ? lo >> (17 + 3 * i) : rest >> (3 * (i - 15))) & 7u);
        if (i < hclen && len) kraft += 128 >> len;
    }
    return kraft == 128;
}

// Whether bit `p` of in[0, in_bytes) is a candidate; `rd` begins at the dword p >> 5.
template <class Reader, class Store> DF_HD bool inf_any_candidate(Reader rd, long long p, long long in_bytes, Store &st) {
    if (p == 0) return in_bytes > 0;
    InfBits<Reader> b(rd);
    const long long limit = in_bytes * 8 - ((p >> 5) << 5);
    b.fill();
    b.drop((int)(p & 31));
    b.fill();
    if (b.take(3) != 4u || b.used() > limit) return false;
    InfDynCodes<Store> codes(st);
    return codes.header(b, limit, limit) == FNN_INFLATE_OK;
}

// The entry a match writes for the source at `src` (a position of the member, negative: before its first byte), `held` the
// entry at that position where src >= 0.
DF_HD unsigned inf_any_entry(long long src, unsigned held) { return src < 0 ? INF_ANY_MARK | (unsigned)(INF_ANY_WINDOW + src) : held; }

// Decodes the member that starts at bit `start` (`rd` begins at the dword start >> 5) and hands the output to the sink,
// position by position from 0:
//   s.literal(pos, v)          one byte
//   s.raw(pos, w, k)           k = 1 .. 4 bytes of a stored block, lowest byte of w first
//   s.match(pos, len, dist)    len = 3 .. 258 entries equal to those dist = 1 .. 32768 back; pos - dist may be negative
// Every call lies inside [0, out_bytes); a refused token is not handed over.  is_cand(bit): whether a candidate begins there.
template <class Reader, class Sink, class Store, class IsCand>
DF_HD InfAnyRecord inf_any_member(Reader rd, long long start, long long in_bytes, long long out_bytes, Sink &s, Store &st, IsCand &is_cand) {
    InfDynCodes<Store> codes(st);
    InfBits<Reader> b(rd);
    const long long base = (start >> 5) << 5, limit = in_bytes * 8 - base;
    long long pos = 0;
    int reach = 0;
    auto stop = [&](int reason) { return InfAnyRecord{-1, pos, reason, reach}; };
    b.fill();
    b.drop((int)(start & 31));
    for (;;) {
        b.fill();
        const unsigned hdr = b.take(3);
        if (b.used() > limit) return stop(FNN_INFLATE_END);
        if ((hdr >> 1) == 3u) return stop(FNN_INFLATE_BTYPE3);
        if ((hdr >> 1) == 0u) {
            b.drop((int)(-b.used() & 7));
            b.fill();
            const unsigned len = b.take(16), nlen = b.take(16);
            if (b.used() > limit) return stop(FNN_INFLATE_END);
            if ((len ^ nlen) != 0xFFFFu) return stop(FNN_INFLATE_NLEN);
            if (pos + (long long)len > out_bytes) return stop(FNN_INFLATE_OUTPUT);
            if (b.used() + 8LL * len > limit) return stop(FNN_INFLATE_END);
            for (int left = (int)len; left > 0;) {
                const int k = left < 4 ? left : 4;
                b.fill();
                s.raw(pos, b.take(8 * k), k);
                pos += k;
                left -= k;
            }
        } else {
            if ((hdr >> 1) == 2u) {
                const int why = codes.header(b, limit, limit);
                if (why != FNN_INFLATE_OK) return stop(why);
            } else {
                codes.begin_fixed();
            }
            for (;;) {
                b.fill();
                int n, extra;
                const int sym = codes.lit(b.peek(15), n);
                b.drop(n);
                if (b.used() > limit) return stop(FNN_INFLATE_END);
                if (sym >= 0 && sym < 256) {
                    if (pos >= out_bytes) return stop(FNN_INFLATE_OUTPUT);
                    s.literal(pos, (unsigned)sym);
                    ++pos;
                    continue;
                }
                if (sym == 256) break;
                if (sym < 0 || sym > 285) return stop(FNN_INFLATE_SYMBOL);
                int len = inf_length_base(sym - 257, extra);
                len += (int)b.take(extra);
                b.fill();
                const int code = codes.dist(b.peek(15), n);
                b.drop(n);
                if (code < 0 || code > 29) return stop(FNN_INFLATE_SYMBOL);
                int dist = inf_distance_base(code, extra);
                dist += (int)b.take(extra);
                if (b.used() > limit) return stop(FNN_INFLATE_END);
                if (pos + len > out_bytes) return stop(FNN_INFLATE_OUTPUT);
                if (dist > pos && (int)(dist - pos) > reach) reach = (int)(dist - pos);
                s.match(pos, len, dist);
                pos += len;
            }
        }
        const long long at = base + b.used();                                   // the block's end
        if (hdr & 1u) {
            if ((at + 7) >> 3 != in_bytes) return stop(FNN_INFLATE_FINAL);
            return InfAnyRecord{in_bytes * 8, pos, FNN_INFLATE_OK, reach};
        }
        if (is_cand(at)) return InfAnyRecord{at, pos, FNN_INFLATE_OK, reach};
    }
}

// the sink of a pass that only judges the member
struct InfAnyNoSink {
    DF_HD void literal(long long, unsigned) {}
    DF_HD void raw(long long, unsigned, int) {}
    DF_HD void match(long long, int, int) {}
};
