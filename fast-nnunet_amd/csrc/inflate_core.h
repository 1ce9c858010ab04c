// inflate_core.h - one segment of a raw deflate stream (RFC 1951) as its decoder sees it, for host and device from the same
// text (tests/inflate_core_host.cpp compiles it for the host): the bit reader, the fixed code by arithmetic, the length and
// distance bases and extras, and the segment rule with its reasons.  The kernels around it are csrc/inflate.hip; the CRC
// arithmetic is deflate_core.h's.  tests/inflate_ref.py restates the rule in Python; the tests compare record for record.
//
// A segment starts at a byte.  It is a run of non-final blocks, each stored (any LEN, LEN / NLEN checked) or fixed Huffman,
// up to and including the first EMPTY stored block, behind which it ends on a byte.  A match reaches back to the segment's
// own first output byte at the most, a segment makes at most FNN_INFLATE_SEGMENT_MAX output bytes and takes at most
// INF_INPUT_MAX input bytes.  That is what the writers of deflate_core.h emit per chunk, and what zlib emits between two
// Z_FULL_FLUSH points with the Z_FIXED strategy.  Anything else ends the decode with one of the FNN_INFLATE_* reasons.
#pragma once
#include "deflate_core.h"
#include "../../include/fnn.h"

static_assert(FNN_INFLATE_SEGMENT_MAX == DF_CHUNK, "a segment is what the encoders call a chunk");

// The input budget of one segment, in bytes.  The two densest ways to state 16384 bytes:
//   9-bit literals in one block: 3 (header) + 9 * 16384 + 7 (end of block) + 3 (stored header) bits, rounded up to a byte,
//     + 4 (LEN, NLEN) = df_chunk_bytes(9 * 16384) = DF_CHUNK_MAX_BYTES = 18438;
//   stored: 1 (header and padding) + 4 + 16384, then the empty block's 1 + 4                                     = 16394.
// A writer may cut either into several blocks; each further block costs at most 5 bytes (a stored header with its padding
// and LEN / NLEN; a fixed block's header and end-of-block code are 10 bits).  Eight further blocks are allowed for, and the
// sum is rounded up to 16: 18438 + 40 -> 18480.
constexpr int INF_INPUT_MAX = (DF_CHUNK_MAX_BYTES + 8 * 5 + 15) / 16 * 16;
static_assert(INF_INPUT_MAX == 18480, "the derivation above");

// what the decode of one candidate leaves: `end` the byte behind the segment in the stream (-1 when it was refused), `len`
// the output bytes made (until the refusal, when there was one), `reason` FNN_INFLATE_OK or why it stopped
struct InfRecord {
    long long end;
    int len;
    int reason;
};

// ---- the bit reader --------------------------------------------------------------------------------------------------
// `Reader::next()` hands out the stream dword by dword, from the aligned dword that holds the segment's first byte on, and
// zeros past the input's end (it never touches memory there).  The reader keeps 33 .. 64 bits after fill(): one token of
// the fixed code takes at most 9 + 5 + 5 + 13 = 32.  used(): the bits dropped since the first dword's bit 0.
template <class Reader> struct InfBits {
    Reader rd;
    unsigned long long acc = 0;
    int n = 0;
    long long taken = 0;
    DF_HD explicit InfBits(Reader r) : rd(r) {}
    DF_HD void fill() {
        if (n <= 32) {
            acc |= (unsigned long long)rd.next() << n;
            n += 32;
            taken += 32;
        }
    }
    DF_HD unsigned peek(int k) const { return (unsigned)acc & (k >= 32 ? 0xFFFFFFFFu : (1u << k) - 1u); }   // k <= 32 <= n
    DF_HD void drop(int k) { acc >>= k; n -= k; }
    DF_HD unsigned take(int k) { const unsigned v = peek(k); drop(k); return v; }
    DF_HD long long used() const { return taken - n; }
};

// the host's reader: the bytes in[at, in_bytes) with `at` a multiple of 4
struct InfBytes {
    const uint8_t *in;
    long long in_bytes, at;
    DF_HD unsigned next() {
        unsigned w = 0;
        for (int k = 0; k < 4; ++k)
            if (at + k < in_bytes) w |= (unsigned)in[at + k] << (8 * k);
        at += 4;
        return w;
    }
};

// ---- the fixed code, by arithmetic -----------------------------------------------------------------------------------
// The next literal / length symbol from the 9 bits `v` (as they lie in the stream, first bit lowest) -> the symbol and, in
// `n`, its bits: 7 for 256 .. 279 (codes 0000000 .. 0010111), 8 for 0 .. 143 (00110000 ..) and 280 .. 287 (11000000 ..),
// 9 for 144 .. 255 (110010000 ..).  The four ranges of 7-bit prefixes - 0 .. 23, 24 .. 95, 96 .. 99, 100 .. 127 - are all there are.
DF_HD int inf_symbol(unsigned v, int &n) {
    const unsigned r9 = df_rev(v & 511u, 9), r7 = r9 >> 2, r8 = r9 >> 1;
    if (r7 < 24) { n = 7; return 256 + (int)r7; }
    if (r7 < 96) { n = 8; return (int)r8 - 0x30; }
    if (r7 < 100) { n = 8; return 280 + (int)r8 - 0xC0; }
    n = 9;
    return 144 + (int)r9 - 0x190;
}

// length symbol 257 + idx (idx 0 .. 28) -> its base and extra bits: 3 .. 10 plain, then four symbols per extra bit, 285 is 258
DF_HD int inf_length_base(int idx, int &extra) {
    extra = 0;
    if (idx < 8) return 3 + idx;
    if (idx == 28) return 258;
    extra = (idx >> 2) - 1;
    return 3 + ((4 + (idx & 3)) << extra);
}

// distance code 0 .. 29 -> its base and extra bits: 1 .. 4 plain, then two codes per extra bit
DF_HD int inf_distance_base(int code, int &extra) {
    extra = 0;
    if (code < 4) return 1 + code;
    extra = (code >> 1) - 1;
    return 1 + ((2 + (code & 1)) << extra);
}

// ---- the two codes a block's tokens are read with -------------------------------------------------------------------------
// What the segment rule asks of them.  `begin_fixed()`: a BTYPE 01 block begins.  `header(b, limit, end_bit)`: a BTYPE 10
// block begins, its table header is next in `b` -> FNN_INFLATE_OK or why the segment stops there.  `lit(v, n)` / `dist(v, n)`:
// the next literal / length or distance symbol from the 15 bits `v` (first bit lowest) and, in `n`, its bits; a negative
// symbol for a bit pattern that belongs to none.  DYNAMIC: a token may take 48 bits, so the reader is filled once more
// before the distance symbol.  These are the codes of this file's rule: BTYPE 10 is refused (inflate_dyn_core.h decodes it).
struct InfFixedCodes {
    static constexpr bool DYNAMIC = false;
    DF_HD void begin_fixed() {}
    template <class Bits> DF_HD int header(Bits &, long long, long long) { return FNN_INFLATE_DYNAMIC; }
    DF_HD int lit(unsigned v, int &n) const { return inf_symbol(v, n); }
    DF_HD int dist(unsigned v, int &n) const { n = 5; return (int)df_rev(v & 31u, 5); }
};

// ---- the segment rule ------------------------------------------------------------------------------------------------
// Decodes the segment that starts at byte `start` of in[0, in_bytes) (`rd` begins at the dword start & ~3) and hands the
// output to the sink, position by position from 0:
//   s.literal(pos, v)          one byte
//   s.raw(pos, w, k)           k = 1 .. 4 bytes of a stored block, lowest byte of w first
//   s.match(pos, len, dist)    len = 3 .. 258 bytes equal to those dist = 1 .. pos back (dist < len: a periodic fill)
// Every call lies inside [0, FNN_INFLATE_SEGMENT_MAX); a refused token is not handed over.
//
// Bound: the limit - the input's end or the budget, whichever comes first - is compared with used() behind everything an
// iteration of the block loop or the token loop drops, and for a stored block before its first byte.  An iteration drops
// at least 3 bits (a block header), 1 (a token; 7 with the fixed code) or 8 (a stored unit of up to 4 bytes), so at most
// 8 * INF_INPUT_MAX + 1 iterations run whatever the input holds, none of them past the limit by more than one token
// (48 bits): the reader is asked for at most three dwords beyond it, which it answers with zeros.
template <class Reader, class Sink, class Codes>
DF_HD InfRecord inf_segment_with(Reader rd, long long start, long long in_bytes, Sink &s, Codes &codes) {
    InfBits<Reader> b(rd);
    const long long first = (start & 3) * 8;                                     // the segment's first bit
    const long long end_bit = (in_bytes - (start & ~3LL)) * 8, budget_bit = first + 8LL * INF_INPUT_MAX;
    const long long limit = end_bit < budget_bit ? end_bit : budget_bit;
    int pos = 0;
    auto stop = [&](int reason) { return InfRecord{-1, pos, reason}; };
    auto over = [&]() { return b.used() > end_bit ? FNN_INFLATE_END : FNN_INFLATE_INPUT; };
    b.fill();
    b.drop((int)first);
    for (;;) {
        b.fill();
        const unsigned hdr = b.take(3);
        if (b.used() > limit) return stop(over());
        if (hdr & 1u) return stop(FNN_INFLATE_FINAL);
        if ((hdr >> 1) == 3u) return stop(FNN_INFLATE_BTYPE3);
        if ((hdr >> 1) == 0u) {
            b.drop((int)(-b.used() & 7));
            b.fill();
            const unsigned len = b.take(16), nlen = b.take(16);
            if (b.used() > limit) return stop(over());
            if ((len ^ nlen) != 0xFFFFu) return stop(FNN_INFLATE_NLEN);
            if (len == 0) return InfRecord{(start & ~3LL) + b.used() / 8, pos, FNN_INFLATE_OK};
            if (pos + (int)len > FNN_INFLATE_SEGMENT_MAX) return stop(FNN_INFLATE_OUTPUT);
            if (b.used() + 8LL * len > limit) return stop(b.used() + 8LL * len > end_bit ? FNN_INFLATE_END : FNN_INFLATE_INPUT);
            for (int left = (int)len; left > 0;) {
                const int k = left < 4 ? left : 4;
                b.fill();
                s.raw(pos, b.take(8 * k), k);
                pos += k;
                left -= k;
            }
            continue;
        }
        if ((hdr >> 1) == 2u) {
            const int why = codes.header(b, limit, end_bit);
            if (why != FNN_INFLATE_OK) return stop(why);
        } else {
            codes.begin_fixed();
        }
        for (;;) {
            b.fill();
            int n, extra;
            const int sym = codes.lit(b.peek(15), n);
            b.drop(n);
            if (b.used() > limit) return stop(over());
            if (sym >= 0 && sym < 256) {
                if (pos >= FNN_INFLATE_SEGMENT_MAX) return stop(FNN_INFLATE_OUTPUT);
                s.literal(pos, (unsigned)sym);
                ++pos;
                continue;
            }
            if (sym == 256) break;
            if (sym < 0 || sym > 285) return stop(FNN_INFLATE_SYMBOL);
            int len = inf_length_base(sym - 257, extra);
            len += (int)b.take(extra);
            if (Codes::DYNAMIC) b.fill();
            const int code = codes.dist(b.peek(15), n);
            b.drop(n);
            if (code < 0 || code > 29) return stop(FNN_INFLATE_SYMBOL);
            int dist = inf_distance_base(code, extra);
            dist += (int)b.take(extra);
            if (b.used() > limit) return stop(over());
            if (dist > pos) return stop(FNN_INFLATE_DISTANCE);
            if (pos + len > FNN_INFLATE_SEGMENT_MAX) return stop(FNN_INFLATE_OUTPUT);
            s.match(pos, len, dist);
            pos += len;
        }
    }
}

// the rule of this file: stored and fixed blocks, FNN_INFLATE_DYNAMIC at the first BTYPE 10
template <class Reader, class Sink> DF_HD InfRecord inf_segment(Reader rd, long long start, long long in_bytes, Sink &s) {
    InfFixedCodes codes;
    return inf_segment_with(rd, start, in_bytes, s, codes);
}

// the sink of a pass that only judges the segment
struct InfNoSink {
    DF_HD void literal(int, unsigned) {}
    DF_HD void raw(int, unsigned, int) {}
    DF_HD void match(int, int, int) {}
};
