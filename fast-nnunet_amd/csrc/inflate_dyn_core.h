// inflate_dyn_core.h - the segment rule of inflate_core.h with one change: a BTYPE 10 block is decoded, not refused.  Host
// and device from the same text (tests/inflate_dyn_core_host.cpp compiles it for the host); the kernels around it are
// csrc/inflate_dyn.hip, tests/inflate_dyn_ref.py restates the rule in Python and the tests compare record for record.
//
// Everything else is kept: a segment is a run of non-final blocks up to and including the first empty stored block, ends on
// a byte, reaches back no further than its own first output byte, makes at most FNN_INFLATE_SEGMENT_MAX bytes and takes at
// most INF_INPUT_MAX input bytes (the project's dynamic chunk is never longer than its fixed chunk, and zlib never emits a
// dynamic block longer than the stored one).  FNN_INFLATE_DYNAMIC is never returned here.
//
// A table header is accepted exactly where zlib's inflate accepts it.  The checks, in this order (every refusal among them
// is FNN_INFLATE_TABLES; the limit is compared behind everything a step drops, as in inflate_core.h, and comes first):
//   1. HLIT = 257 + 5 bits <= 286 and HDIST = 1 + 5 bits <= 30, behind the 14 bits of HLIT, HDIST and HCLEN;
//   2. the HCLEN + 4 three-bit lengths, in the permuted order, are a complete code: neither over-subscribed nor
//      incomplete (a single code, or none at all, is incomplete);
//   3. the HLIT + HDIST lengths, one sequence: 16 repeats the length before it 3 .. 6 times and is refused at position 0,
//      17 gives 3 .. 10 zeros, 18 gives 11 .. 138; a run that overshoots HLIT + HDIST is refused;
//   4. the length of symbol 256 is not 0;
//   5. the literal / length set, then the distance set: not over-subscribed, and incomplete only with no code longer than
//      1 bit (one code of length 1; for the distance set also no code at all: a block of literals only).
// A bit pattern that belongs to no symbol of an accepted incomplete set takes 1 bit and is FNN_INFLATE_SYMBOL.
//
// The bit reader: a dynamic token takes up to 15 + 5 + 15 + 13 = 48 bits and InfBits guarantees 33 after fill(), so the
// token loop fills once before the literal / length symbol (15 + 5) and once before the distance symbol (15 + 13); a step
// of the table header drops at most 7 + 7 = 14 bits behind one fill.  The limit is compared behind every step, so no step
// goes past it by more than the 48 bits of a token, and - 64 bits at the most being held - the reader is asked for at
// most three dwords past the limit, which it answers with zeros.
//
// Loops: the table header takes at most 19 + 316 steps; a token drops at least 1 bit, so the token loops of a segment run at
// most 8 * INF_INPUT_MAX times together whatever the input holds.
//
// How a code's tables are stored and built is the caller's `Store` (the host harness: serially in plain arrays; the
// kernels: by the wave, in LDS).  The codes are canonical (RFC 1951 3.2.2) and decoded as such: per length l the first
// code, the number of codes and the place of the length's first symbol in the list of symbols sorted by (length, symbol).
// The rule here takes the counts, makes the Kraft check and the verdict, and hands each length its three numbers; the
// Store counts, sorts and looks up:
//   st.set_len(i, len)                 length i of the block's sequence, i < INF_DYN_LENS; the code-length code's own 19
//   st.set_run(i, rep, len)              lengths are the sequence's entries INF_DYN_CL_AT ..
//   st.template count<W>(lo, n)        counts, per length, the entries [lo, lo + n) of the sequence for code W
//   st.template count_of<W>(l)         -> the number of codes of length l = 1 .. 15
//   st.template set_code<W>(l, first, count, place)
//   st.template sort<W>(lo, n)         the sorted list of code W, from the counts and places
//   st.template symbol<W>(v, n)        the symbol of the 15 bits v (first bit lowest) and, in n, its bits; -1 and 1 bit
//                                      for a pattern that belongs to none
// A Store forms every index from stream bits so that it is bounded by construction (a masked place in a power-of-two
// list): no input addresses outside its tables.
#pragma once
#include "inflate_core.h"

constexpr int INF_CODE_CL = 0, INF_CODE_LIT = 1, INF_CODE_DIST = 2;
constexpr int INF_DYN_LENS = 286 + 30;                  // the most lengths a block's sequence holds
constexpr int INF_DYN_CL_AT = 320;                      // where the code-length code's 19 lengths lie behind them
constexpr int INF_DYN_SEQ = INF_DYN_CL_AT + 32;         // the entries of the sequence a Store keeps

// the permuted order of the code-length code's lengths, 5 bits each: 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
DF_HD int inf_cl_order(int i) {
    const unsigned long long lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                                  10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const unsigned long long hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// Code W from the entries [lo, lo + n) of the sequence -> whether it is accepted: never an over-subscribed set; an
// incomplete one only where `may_be_short` and no code is longer than 1 bit.
template <int W, class Store> DF_HD bool inf_build_code(Store &st, int lo, int n, bool may_be_short) {
    st.template count<W>(lo, n);
    int left = 1, first = 0, place = 0, longest = 0;
    for (int l = 1; l <= 15; ++l) {
        const int c = st.template count_of<W>(l);
        left = 2 * left - c;
        if (left < 0) return false;
        st.template set_code<W>(l, first, c, place);
        first = (first + c) << 1;
        place += c;
        if (c) longest = l;
    }
    if (left > 0 && !(may_be_short && longest <= 1)) return false;
    st.template sort<W>(lo, n);
    return true;
}

template <class Store> struct InfDynCodes {
    static constexpr bool DYNAMIC = true;
    Store &st;
    bool dynamic = false;                                // the block being decoded: BTYPE 10, else 01
    DF_HD explicit InfDynCodes(Store &s) : st(s) {}
    DF_HD void begin_fixed() { dynamic = false; }
    DF_HD int lit(unsigned v, int &n) const { return dynamic ? st.template symbol<INF_CODE_LIT>(v, n) : inf_symbol(v, n); }
    DF_HD int dist(unsigned v, int &n) const {
        if (dynamic) return st.template symbol<INF_CODE_DIST>(v, n);
        n = 5;
        return (int)df_rev(v & 31u, 5);
    }
    template <class Bits> DF_HD int header(Bits &b, long long limit, long long end_bit) {
        auto over = [&]() { return b.used() > end_bit ? FNN_INFLATE_END : FNN_INFLATE_INPUT; };
        dynamic = true;
        b.fill();
        const int hlit = 257 + (int)b.take(5), hdist = 1 + (int)b.take(5), hclen = 4 + (int)b.take(4);
        if (b.used() > limit) return over();
        if (hlit > 286 || hdist > 30) return FNN_INFLATE_TABLES;
        for (int i = 0; i < 19; ++i) {
            int len = 0;
            if (i < hclen) {
                b.fill();
                len = (int)b.take(3);
                if (b.used() > limit) return over();
            }
            st.set_len(INF_DYN_CL_AT + inf_cl_order(i), len);
        }
        if (!inf_build_code<INF_CODE_CL>(st, INF_DYN_CL_AT, 19, false)) return FNN_INFLATE_TABLES;
        const int total = hlit + hdist;
        int prev = 0, eob = 0;
        for (int i = 0; i < total;) {
            b.fill();
            int n, rep = 1, len;
            const int sym = st.template symbol<INF_CODE_CL>(b.peek(15), n);   // (the code is complete: never negative)
            b.drop(n);
            if (sym < 16) len = sym < 0 ? 0 : sym;
            else if (sym == 16) { len = prev; rep = 3 + (int)b.take(2); }
            else if (sym == 17) { len = 0; rep = 3 + (int)b.take(3); }
            else { len = 0; rep = 11 + (int)b.take(7); }
            if (b.used() > limit) return over();
            if (sym < 0 || (sym == 16 && i == 0) || i + rep > total) return FNN_INFLATE_TABLES;
            if (rep == 1) st.set_len(i, len);
            else st.set_run(i, rep, len);
            if (i <= 256 && 256 < i + rep) eob = len;
            prev = len;
            i += rep;
        }
        if (eob == 0) return FNN_INFLATE_TABLES;
        if (!inf_build_code<INF_CODE_LIT>(st, 0, hlit, true)) return FNN_INFLATE_TABLES;
        if (!inf_build_code<INF_CODE_DIST>(st, hlit, hdist, true)) return FNN_INFLATE_TABLES;
        return FNN_INFLATE_OK;
    }
};

template <class Reader, class Sink, class Store>
DF_HD InfRecord inf_dyn_segment(Reader rd, long long start, long long in_bytes, Sink &s, Store &st) {
    InfDynCodes<Store> codes(st);
    return inf_segment_with(rd, start, in_bytes, s, codes);
}

// ---- the host's Store: plain arrays, built serially -------------------------------------------------------------------
struct InfHostStore {
    uint8_t seq[INF_DYN_SEQ] = {};
    int cnt[3][16] = {}, first[3][16] = {}, place[3][16] = {};
    uint16_t sorted[3][512] = {};
    void set_len(int i, int len) { seq[i] = (uint8_t)len; }
    void set_run(int i, int rep, int len) { for (int j = 0; j < rep; ++j) seq[i + j] = (uint8_t)len; }
    template <int W> void count(int lo, int n) {
        for (int l = 0; l < 16; ++l) cnt[W][l] = 0;
        for (int s = 0; s < n; ++s) ++cnt[W][seq[lo + s] & 15];
    }
    template <int W> int count_of(int l) const { return cnt[W][l]; }
    template <int W> void set_code(int l, int f, int c, int p) { first[W][l] = f; cnt[W][l] = c; place[W][l] = p; }
    template <int W> void sort(int lo, int n) {
        int next[16];
        for (int l = 0; l < 16; ++l) next[l] = place[W][l];
        for (int s = 0; s < n; ++s)
            if (const int l = seq[lo + s] & 15) sorted[W][next[l]++ & 511] = (uint16_t)s;
    }
    template <int W> int symbol(unsigned v, int &n) const {
        const int code = (int)df_rev(v & 0x7FFFu, 15);           // the 15 bits as a code, first bit highest
        for (int l = 1; l <= 15; ++l) {
            const int c = code >> (15 - l);
            if (c < first[W][l] + cnt[W][l]) {                   // (>= first[W][l]: it was not below the length before)
                n = l;
                return sorted[W][(place[W][l] + c - first[W][l]) & 511];
            }
        }
        n = 1;
        return -1;
    }
};
