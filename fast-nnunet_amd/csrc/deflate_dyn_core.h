// deflate_dyn_core.h - the per-chunk dynamic Huffman tables of csrc/deflate_dyn.hip, for host and device from the same text
// (tests/deflate_dyn_host.cpp compiles it for the host); tests/deflate_dyn_ref.py restates the rule in Python and the tests
// compare byte for byte.  Tokens, segments, chunks and the framing are deflate_core.h's.
//
// A chunk is one non-final block, its end-of-block code and an empty stored block.  The block is BTYPE 10 with the chunk's
// own tables where that takes fewer bits than BTYPE 01 (deflate_core.h's fixed code); a tie goes to the fixed code.  So no
// chunk is longer than the fixed code's, and a fragment stays a chain of independent byte-aligned chunks that each end
// behind 00 00 FF FF.
//
// * Frequencies: the literal / length symbols of the chunk's tokens, and one for 256.  Invariant: a non-empty chunk uses
//   at least two symbols - the first byte of a segment is always a literal, and 256.
// * The distance code is constant: symbols 0 and 1, both of length 1 (HDIST = 2 codes).  It is complete, so no decoder has
//   to accept an incomplete code, and a match's distance costs one bit.
// * df_code_lengths(freq, n, limit, len): a Huffman tree from two queues - the used symbols ascending by (frequency,
//   index), and the merged nodes in the order they are made; the smaller head is taken, the merged node on a tie.  The
//   leaves' depths, those above `limit` counted as `limit`, are a multiset of lengths whose Kraft sum may exceed 1 by a
//   multiple e of 2^-limit.  e times, the deepest leaf above the last level moves one level down and a leaf of the last
//   level becomes its brother: that takes exactly 2^-limit off the sum, and a leaf of the last level always remains (the
//   e clamped leaves each add less than 2^-limit).  The lengths are handed out longest first to the symbols in ascending
//   order.  Length 0 goes exactly to frequency 0; with two or more used symbols Kraft holds with equality; one used symbol
//   gets length 1.  A tree deeper than `limit` gives a longest length of exactly `limit`.  Taking the merged node on a tie
//   gives the deepest of the equally cheap trees, so the limit applies more often than with the leaf first, and the
//   repaired lengths are complete but not the optimal length-limited code: optimality under the limit is not claimed.
// * Codes are canonical (RFC 1951 3.2.2).  HLIT = max(257, last used symbol + 1).
// * The HLIT + 2 lengths - literal / length, then the two distance lengths, as one sequence, so a run may cross from the
//   one into the other - are coded greedily from the left.  At position i with value v and r equal values from i on:
//     v = 0: r >= 11 -> 18 with min(r, 138); r >= 3 -> 17 with r; else the length 0 itself
//     v > 0: i > 0, the value before i is v and r >= 3 -> 16 with min(r, 6); else the length v itself
// * The code-length code is df_code_lengths(., 19, 7, .); HCLEN is trimmed along the permuted order and is at least 4.
//
// The functions below that take a `Par` are run by all lanes of a wave together (DfSerial: by the one thread of the host):
// lane() of lanes() shares the loops over symbols, sync() is a barrier behind which what the others wrote is read.  Their
// control flow depends on shared values alone.  Every loop has a bound written next to it.
#pragma once
#include "deflate_core.h"

constexpr int DF_NLIT = 286;                    // literal / length symbols
constexpr int DF_NLIT_PAD = 288;                // ... and the sequence of the header: up to 286 + 2 lengths
constexpr int DF_NCL = 19;                      // symbols of the code-length code
constexpr int DF_LIT_LIMIT = 15, DF_CL_LIMIT = 7;
// the table header: 3 + 5 + 5 + 4 bits, 19 x 3, and at most 288 code-length symbols of at most 7 bits (16 / 17 / 18 carry
// up to 7 more but stand for 3 positions or more): 2090 bits
constexpr int DF_HDR_DWORDS = 68;
constexpr int DF_LEN_DWORDS = DF_NLIT_PAD / 8;  // the literal / length lengths, 4 bits each
constexpr int DF_DYN_REC_DWORDS = DF_LEN_DWORDS + DF_HDR_DWORDS;   // what the count pass keeps per chunk for the emit pass

struct DfSerial {
    DF_HD int lane() const { return 0; }
    DF_HD int lanes() const { return 1; }
    DF_HD void sync() const {}
};

struct DfHuffWork {
    uint32_t w[DF_NLIT_PAD];                    // the merged nodes' weights
    uint16_t order[DF_NLIT_PAD];                // the used symbols, ascending by (frequency, index)
    uint16_t up[2 * DF_NLIT_PAD];               // node -> the node above it; then node -> its depth.  Leaves 0 .. used - 1
    uint32_t count[16];                         // the leaves of each length
    int used;
};

// n <= 286 symbols of frequencies that sum to less than 2^31, limit 7 or 15 (2^limit > n: a last level can hold all leaves)
template <class Par>
DF_HD void df_code_lengths(const uint32_t *freq, int n, int limit, uint8_t *len, DfHuffWork &k, Par par) {
    if (par.lane() == 0) k.used = 0;
    for (int s = par.lane(); s < n; s += par.lanes()) len[s] = 0;
    par.sync();
    for (int s = par.lane(); s < n; s += par.lanes()) {                      // bound: n
        const uint32_t fs = freq[s];
        if (!fs) continue;
        int rank = 0, cnt = 0;
        for (int t = 0; t < n; ++t) {                                        // bound: n
            const uint32_t ft = freq[t];
            cnt += ft != 0;
            rank += ft != 0 && (ft < fs || (ft == fs && t < s));
        }
        k.order[rank] = (uint16_t)s;
        if (rank == cnt - 1) k.used = cnt;                                   // (the last in order says how many there are)
    }
    par.sync();
    const int m = k.used;
    if (par.lane() == 0 && m == 1) len[k.order[0]] = 1;
    if (par.lane() == 0 && m >= 2) {
        // nodes 0 .. m - 1: the leaves in order; m .. 2 m - 2: the merged nodes as they are made, the last the root
        int leaf = 0, node = m, made = m;
        for (int i = 0; i < m - 1; ++i) {                                    // bound: m - 1 <= 285
            uint32_t sum = 0;
            for (int j = 0; j < 2; ++j) {
                const bool take_leaf = leaf < m && (node >= made || freq[k.order[leaf]] < k.w[node - m]);
                const int t = take_leaf ? leaf++ : node++;
                sum += take_leaf ? freq[k.order[t]] : k.w[t - m];
                k.up[t] = (uint16_t)made;
            }
            k.w[made - m] = sum;
            ++made;
        }
        for (int l = 0; l < 16; ++l) k.count[l] = 0;
        k.up[2 * m - 2] = 0;
        for (int i = 2 * m - 3; i >= 0; --i) {                               // bound: 2 m - 2 <= 570; up[i] > i is a depth already
            const int d = k.up[k.up[i]] + 1;
            k.up[i] = (uint16_t)d;
            if (i < m) ++k.count[d < limit ? d : limit];
        }
        uint32_t kraft = 0;                                                  // in units of 2^-limit
        for (int l = 1; l <= limit; ++l) kraft += k.count[l] << (limit - l);
        for (int e = 0; e < m && kraft > (1u << limit); ++e) {               // bound: m (the excess is below the clamped leaves)
            int b = limit - 1;
            while (b > 1 && k.count[b] == 0) --b;                            // bound: limit
            if (k.count[b] == 0 || k.count[limit] == 0) break;               // (never: see the rule)
            --k.count[b];
            k.count[b + 1] += 2;
            --k.count[limit];
            --kraft;
        }
        int i = 0;
        for (int l = limit; l >= 1; --l)
            for (uint32_t c = k.count[l]; c > 0 && i < m; --c) len[k.order[i++]] = (uint8_t)l;   // bound: m in all
    }
    par.sync();
}

// RFC 1951 3.2.2: lengths (<= 15) -> per used symbol its code as the bits go into the stream | length << 16; `next`: 16 dwords
template <class Par>
DF_HD void df_canonical(const uint8_t *len, int n, uint32_t *packed, uint32_t *next, Par par) {
    for (int l = par.lane(); l < 16; l += par.lanes()) {                     // next[l]: the symbols of length l
        uint32_t c = 0;
        for (int t = 0; t < n; ++t) c += l > 0 && len[t] == l;               // bound: n
        next[l] = c;
    }
    par.sync();
    if (par.lane() == 0) {
        uint32_t code = 0, before = 0;
        for (int l = 1; l < 16; ++l) {                                       // next[l]: the first code of length l
            code = (code + before) << 1;
            before = next[l];
            next[l] = code;
        }
    }
    par.sync();
    for (int s = par.lane(); s < n; s += par.lanes()) {
        const int l = len[s];
        uint32_t code = next[l & 15];
        if (l) for (int t = 0; t < s; ++t) code += len[t] == l;             // bound: n
        packed[s] = l ? df_rev(code, l) | (uint32_t)l << 16 : 0u;
    }
    par.sync();
}

// a match length (3 .. 258) -> its symbol, the number of its extra bits and their value
DF_HD void df_length_symbol(int len, int &sym, int &eb, unsigned &extra) {
    const int l = len - 3;
    eb = 0;
    extra = 0;
    if (l < 8) sym = 257 + l;
    else if (len == 258) sym = 285;
    else {
        eb = 29 - __builtin_clz((unsigned)l);                                // floor(log2(l)) - 2: 1 .. 5
        sym = 261 + 4 * eb + ((l >> eb) & 3);
        extra = (unsigned)l & ((1u << eb) - 1);
    }
}
// the bits a literal / length symbol takes behind its code: a length's extra bits and its distance's one bit
DF_HD int df_symbol_tail(int sym) { return sym <= 256 ? 0 : 1 + (sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2); }

// ---- the tables of one chunk ------------------------------------------------------------------------------------------
struct DfDynWork {
    DfHuffWork huff;
    uint32_t freq[DF_NLIT_PAD];                 // the chunk's literal / length symbols
    uint8_t len[DF_NLIT_PAD];                   // their code lengths, followed (header) by the two distance lengths
    uint16_t tok[DF_NLIT_PAD];                  // the header's code-length symbols: symbol | extra value << 5
    uint32_t cl_freq[DF_NCL];
    uint8_t cl_len[DF_NCL + 1];
    uint32_t cl_code[DF_NCL];
    uint32_t next[16];
    uint32_t hdr[DF_HDR_DWORDS];                // BFINAL, BTYPE and the table header, as the bits go into the stream
    int n_tok, hlit, hdr_bits;
};

DF_HD int df_cl_extra_bits(int sym) { return sym == 16 ? 2 : (sym == 17 ? 3 : (sym == 18 ? 7 : 0)); }

// plain bits into a zeroed buffer (one lane)
struct DfPut {
    uint32_t *buf;
    int pos = 0;
    DF_HD void put(unsigned v, int nb) {                                     // nb <= 16
        const unsigned long long x = (unsigned long long)v << (pos & 31);
        buf[pos >> 5] |= (uint32_t)x;
        if ((pos & 31) + nb > 32) buf[(pos >> 5) + 1] |= (uint32_t)(x >> 32);
        pos += nb;
    }
};

// k.freq -> k.len, k.hdr, k.hdr_bits
template <class Par> DF_HD void df_dyn_tables(DfDynWork &k, Par par) {
    static_assert(DF_NLIT + 2 <= DF_NLIT_PAD, "the header's sequence");
    const uint8_t order[DF_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    df_code_lengths(k.freq, DF_NLIT, DF_LIT_LIMIT, k.len, k.huff, par);
    for (int s = DF_NLIT + par.lane(); s < DF_NLIT_PAD; s += par.lanes()) k.len[s] = 0;
    for (int s = par.lane(); s < DF_NCL; s += par.lanes()) k.cl_freq[s] = 0;
    for (int s = par.lane(); s < DF_HDR_DWORDS; s += par.lanes()) k.hdr[s] = 0;
    par.sync();
    if (par.lane() == 0) {
        int hlit = DF_NLIT;
        while (hlit > 257 && k.len[hlit - 1] == 0) --hlit;                   // bound: 29
        const uint8_t after0 = k.len[hlit], after1 = k.len[hlit + 1];        // (hlit + 1 <= 287)
        k.len[hlit] = k.len[hlit + 1] = 1;                                   // the distance lengths follow in the sequence
        const int n = hlit + 2;
        int i = 0, nt = 0;
        while (i < n) {                                                      // bound: n <= 288, i grows by r >= 1
            const int v = k.len[i];
            int r = 1;
            while (i + r < n && k.len[i + r] == v) ++r;                      // bound: n
            int sym = v, extra = 0;
            if (v == 0 && r >= 11) { r = r > 138 ? 138 : r; sym = 18; extra = r - 11; }
            else if (v == 0 && r >= 3) { sym = 17; extra = r - 3; }
            else if (v != 0 && i > 0 && k.len[i - 1] == v && r >= 3) { r = r > 6 ? 6 : r; sym = 16; extra = r - 3; }
            else r = 1;
            k.tok[nt++] = (uint16_t)(sym | extra << 5);
            ++k.cl_freq[sym];
            i += r;
        }
        k.len[hlit] = after0;
        k.len[hlit + 1] = after1;
        k.n_tok = nt;
        k.hlit = hlit;
    }
    par.sync();
    df_code_lengths(k.cl_freq, DF_NCL, DF_CL_LIMIT, k.cl_len, k.huff, par);
    df_canonical(k.cl_len, DF_NCL, k.cl_code, k.next, par);
    if (par.lane() == 0) {
        int hclen = DF_NCL;
        while (hclen > 4 && k.cl_len[order[hclen - 1]] == 0) --hclen;        // bound: 15
        DfPut b{k.hdr};
        b.put(4u, 3);                                                        // BFINAL = 0, BTYPE = 10
        b.put((unsigned)(k.hlit - 257), 5);
        b.put(1u, 5);                                                        // HDIST = 2
        b.put((unsigned)(hclen - 4), 4);
        for (int i = 0; i < hclen; ++i) b.put(k.cl_len[order[i]], 3);
        for (int i = 0; i < k.n_tok; ++i) {                                  // bound: n_tok <= 288
            const int sym = k.tok[i] & 31;
            const uint32_t c = k.cl_code[sym];
            b.put(c & 0xFFFFu, (int)(c >> 16));
            b.put((unsigned)(k.tok[i] >> 5), df_cl_extra_bits(sym));
        }
        k.hdr_bits = b.pos;
    }
    par.sync();
}

// this lane's share of the bits the chunk's tokens and its end-of-block code take under k.len
template <class Par> DF_HD unsigned df_dyn_token_bits(const DfDynWork &k, Par par) {
    unsigned bits = 0;
    for (int s = par.lane(); s < DF_NLIT; s += par.lanes()) bits += k.freq[s] * (unsigned)(k.len[s] + df_symbol_tail(s));
    return bits;
}

// the chunk's bytes from the bits of its block (header, tokens, end-of-block) of either kind
DF_HD unsigned df_block_chunk_bytes(unsigned block_bits) { return (block_bits + 3 + 7) / 8 + 4; }

// ---- the lanes' walks -------------------------------------------------------------------------------------------------
// walk 1: the fixed code's bits and the CRC-32 as DfCount, and the symbols into the histogram.  The running symbol's count
// is held back and added when the symbol changes: in a constant chunk all lanes count the same two symbols.
template <int DIST> struct DfDynCount {
    DfCount<DIST> fixed;
    uint32_t *freq;
    int cur = -1;
    unsigned n = 0;
    DF_HD void add(uint32_t *p, unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
        atomicAdd(p, v);
#else
        *p += v;
#endif
    }
    DF_HD void symbol(int s) {
        if (s == cur) { ++n; return; }
        if (n) add(freq + cur, n);
        cur = s;
        n = 1;
    }
    DF_HD void finish() { if (n) add(freq + cur, n); n = 0; }
    DF_HD void byte(unsigned b) { fixed.byte(b); }
    DF_HD void literal(unsigned v) { fixed.literal(v); symbol((int)v); }
    DF_HD void match(int len) {
        fixed.match(len);
        int sym, eb;
        unsigned extra;
        df_length_symbol(len, sym, eb, extra);
        symbol(sym);
    }
};

// walk 2: the segment's bits under the chunk's code
struct DfDynBits {
    const uint8_t *len;
    unsigned bits = 0;
    DF_HD void byte(unsigned) {}
    DF_HD void literal(unsigned v) { bits += len[v]; }
    DF_HD void match(int l) {
        int sym, eb;
        unsigned extra;
        df_length_symbol(l, sym, eb, extra);
        bits += len[sym] + eb + 1;
    }
};

// the emit pass: the codes of df_canonical, put by DfEmit's writer
template <int DIST> struct DfDynEmit {
    DfEmit<DIST> em;
    const uint32_t *code;
    DF_HD void byte(unsigned) {}
    DF_HD void symbol(int s) { const uint32_t c = code[s]; em.put(c & 0xFFFFu, (int)(c >> 16)); }
    DF_HD void literal(unsigned v) { symbol((int)v); }
    DF_HD void match(int len) {
        int sym, eb;
        unsigned extra;
        df_length_symbol(len, sym, eb, extra);
        symbol(sym);
        em.put(extra | (DIST == 2 ? 1u : 0u) << eb, eb + 1);                 // the extra bits, the one-bit distance code
    }
};

// the lengths as the count pass keeps them, 4 bits each
DF_HD uint32_t df_pack_lengths(const uint8_t *len, int dword) {
    uint32_t v = 0;
    for (int i = 0; i < 8; ++i) v |= (uint32_t)(len[dword * 8 + i] & 15u) << (4 * i);
    return v;
}
