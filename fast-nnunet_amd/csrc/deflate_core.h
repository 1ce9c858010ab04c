// deflate_core.h - the stream format of the deflate encoders (csrc/deflate.hip, csrc/deflate_masks.hip) as one lane sees it,
// for host and device from the same text (tests/deflate_core_host.cpp compiles it for the host): the token rule and its two
// readers, the fixed-Huffman codes, the bit counter and the bit writer, the CRC-32 field arithmetic and the zero chunk of
// the per-label masks.  What a wave does with its lanes' results is csrc/deflate_wave.h.
// tests/deflate_ref.py and tests/deflate_masks_ref.py restate the format in Python; the tests compare byte for byte.
//
// A fragment is a concatenation of independent chunks of DF_CHUNK = 16 KiB of input bytes.  A chunk is one non-final
// fixed-Huffman block (RFC 1951 3.2.6), its end-of-block code and an empty stored block (000, pad, 00 00 FF FF), which
// ends it on a byte; no match reaches outside its chunk.  Lane l of a wave tokenises the DF_SEG = 256 bytes
// [256 l, 256 l + 256) of the chunk on its own.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define DF_HD __host__ __device__ __forceinline__
#else
#define DF_HD inline
#endif

constexpr int DF_SEG = 256;                     // input bytes a lane tokenises on its own
constexpr int DF_LANES = 64;
constexpr int DF_CHUNK = DF_SEG * DF_LANES;     // input bytes of one wave: one independent, byte-aligned piece of the stream
constexpr int DF_PITCH = DF_SEG / 4 + 1;        // dwords between two segments in LDS: odd, so that lane l's dword i lies on bank
                                                // (l + i) % 32 and the 32 lanes ds_read_b32 serves at once fall on 32 banks
constexpr uint32_t DF_POLY = 0xEDB88320u;       // CRC-32, reflected
constexpr int DF_FRAME_BITS = 3 + 7 + 3;        // block header, end-of-block code, header of the empty stored block
static_assert(DF_SEG <= 258, "a run inside one segment must fit one match");

// the bytes of a chunk whose tokens take `bits`: the framing rounded up to a byte, 00 00 FF FF
constexpr DF_HD unsigned df_chunk_bytes(unsigned bits) { return (bits + DF_FRAME_BITS + 7) / 8 + 4; }
constexpr int DF_CHUNK_MAX_BYTES = (int)df_chunk_bytes(DF_CHUNK * 9);        // every byte a 9-bit literal
constexpr int DF_MASK_CHUNK_MAX_BYTES = (int)df_chunk_bytes(DF_CHUNK * 8);   // a mask's bytes are 0 and 1, 8-bit literals

inline size_t df_align16(size_t v) { return (v + 15) & ~(size_t)15; }

// ---- CRC-32 field arithmetic ---------------------------------------------------------------------------------------
// a * b modulo the CRC-32 polynomial in the reflected representation (bit 31 is x^0)
DF_HD uint32_t df_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1) ? DF_POLY : 0u);
    }
    return p;
}

// x2k[k] = x^(2^k) modulo the polynomial (host; the kernels read a copy)
struct DfTables {
    uint32_t x2k[64];
    DfTables() {
        x2k[0] = 0x40000000u;
        for (int k = 1; k < 64; ++k) x2k[k] = df_mulmod(x2k[k - 1], x2k[k - 1]);
    }
};

// x^(8 n_bytes): repeated squaring, one product per set bit of the exponent
DF_HD uint32_t df_xpow8(unsigned long long n_bytes, const uint32_t *x2k) {
    uint32_t r = 0;
    unsigned long long e = n_bytes;
    for (int k = 3; e; ++k, e >>= 1)
        if (e & 1) r = r ? df_mulmod(r, x2k[k]) : x2k[k];
    return r ? r : 0x80000000u;
}

// The CRC chain: crc(A | B) = crc(A) x^(8 |B|) + crc(B).  `crc` covers what came so far, `next` the `len` bytes that follow;
// x_chunk = df_xpow8(DF_CHUNK, x2k), the power nearly every unit of a chain of chunks takes, computed once by the caller.
DF_HD uint32_t df_crc_append(uint32_t crc, uint32_t next, unsigned long long len, const uint32_t *x2k, uint32_t x_chunk) {
    return df_mulmod(crc, len == DF_CHUNK ? x_chunk : df_xpow8(len, x2k)) ^ next;
}

// ---- the fixed code --------------------------------------------------------------------------------------------------
DF_HD unsigned df_rev(unsigned v, int n) {
#if defined(__clang__)
    return __builtin_bitreverse32(v) >> (32 - n);
#else
    unsigned r = 0;
    for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
#endif
}

// the fixed code of a literal byte, as the bits go into the stream
DF_HD void df_literal(unsigned v, unsigned &code, int &n) {
    if (v < 144) { code = df_rev(0x30 + v, 8); n = 8; }
    else { code = df_rev(0x190 + v - 144, 9); n = 9; }
}

// a match of `len` (3 .. 258) at distance DIST = 1 or 2 bytes (distance codes 0 and 1, five bits, no extra bits): length
// symbol, its extra bits, distance code
template <int DIST> DF_HD void df_match(int len, unsigned &code, int &n) {
    int sym, eb = 0;
    unsigned extra = 0;
    const int l = len - 3;
    if (l < 8) sym = 257 + l;
    else if (len == 258) sym = 285;
    else {
        eb = 29 - __builtin_clz((unsigned)l);           // floor(log2(l)) - 2: 1 .. 5
        sym = 261 + 4 * eb + ((l >> eb) & 3);
        extra = (unsigned)l & ((1u << eb) - 1);
    }
    if (sym < 280) { code = df_rev(sym - 256, 7); n = 7; }
    else { code = df_rev(0xC0 + sym - 280, 8); n = 8; }
    code |= extra << n;
    n += eb;
    code |= (DIST == 2 ? 16u : 0u) << n;                 // the 5-bit distance code, reversed
    n += 5;
}

// ---- the token rule --------------------------------------------------------------------------------------------------
// A byte that equals the byte DIST before it (inside the segment) extends the current run; a run of 3 or more is one
// match, a shorter one its literals.  The greedy statement of tests/deflate_ref.py gives the same tokens, because a run
// never exceeds DF_SEG - DIST < 258.  `rd(q)` yields byte q of the segment, for q = 0 .. len - 1 in order; `len` <= DF_SEG.
template <int DIST, class Reader, class Sink> DF_HD void df_walk(Reader rd, int len, Sink &s) {
    int run = 0;
    unsigned h1 = 0, h2 = 0;                             // the two bytes before q
    auto flush = [&]() {
        if (run >= 3) s.match(run);
        else if (run == 2) { s.literal(h2); s.literal(h1); }
        else if (run == 1) s.literal(h1);
    };
    for (int q = 0; q < len; ++q) {
        const unsigned b = rd(q);
        s.byte(b);
        if (q >= DIST && b == (DIST == 1 ? h1 : h2)) ++run;
        else { flush(); s.literal(b); run = 0; }
        h2 = h1;
        h1 = b;
    }
    flush();
}

// The readers keep the dword they are in, so that each dword of the segment (`seg`) is loaded once.
// The file bytes of a label map, packed: walked with DIST = the bytes of an element.
struct DfBytes {
    const unsigned *seg;
    unsigned w = 0;
    DF_HD unsigned operator()(int q) {
        if ((q & 3) == 0) w = seg[q >> 2];
        const unsigned b = w & 255u;
        w >>= 8;
        return b;
    }
};
// The bytes of the mask m[i] = (seg[i] == label), compared on read: `seg` holds labels of E bytes (all 16 bits of a 2-byte
// label are compared) and no mask byte is stored.  Walked with DIST = 1.
template <int E> struct DfMask {
    const unsigned *seg;
    unsigned label;
    unsigned w = 0;
    DF_HD unsigned operator()(int q) {
        if ((q & (4 / E - 1)) == 0) w = seg[q / (4 / E)];
        const unsigned v = w & (E == 1 ? 255u : 0xFFFFu);
        w >>= 8 * E;
        return v == label ? 1u : 0u;
    }
};

// pass 1: the bits a segment takes and, with CRC, its CRC-32 (tab: the 256-entry byte table)
template <int DIST, bool CRC = true> struct DfCount {
    const uint32_t *tab = nullptr;
    unsigned bits = 0;
    uint32_t crc = 0xFFFFFFFFu;
    DF_HD void byte(unsigned b) { if (CRC) crc = tab[(crc ^ b) & 255u] ^ (crc >> 8); }
    DF_HD void literal(unsigned v) { bits += v < 144 ? 8 : 9; }
    DF_HD void match(int len) { unsigned c; int n; df_match<DIST>(len, c, n); bits += n; }
};

// pass 2: the bits themselves, OR-ed into a zeroed buffer from bit `pos` on.  Neighbouring lanes share the dword in which
// one's bits end and the next one's begin: the OR is atomic on the device, and its result does not depend on the order.
template <int DIST> struct DfEmit {
    unsigned *buf;
    int w, n;
    unsigned long long acc = 0;
    DF_HD DfEmit(unsigned *b, unsigned pos) : buf(b), w((int)(pos >> 5)), n((int)(pos & 31)) {}
    DF_HD void word_or(unsigned *p, unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
        atomicOr(p, v);
#else
        *p |= v;
#endif
    }
    DF_HD void put(unsigned v, int nb) {                 // n < 32 and nb <= 18
        acc |= (unsigned long long)v << n;
        n += nb;
        if (n >= 32) { word_or(buf + w, (unsigned)acc); ++w; acc >>= 32; n -= 32; }
    }
    DF_HD void finish() { if (n > 0) word_or(buf + w, (unsigned)acc); }
    DF_HD void byte(unsigned) {}
    DF_HD void literal(unsigned v) { unsigned c; int nb; df_literal(v, c, nb); put(c, nb); }
    DF_HD void match(int len) { unsigned c; int nb; df_match<DIST>(len, c, nb); put(c, nb); }
};

// ---- per-label masks -------------------------------------------------------------------------------------------------
// The mask's fragment is the chain of chunks above with one change: a full chunk in which the label does not occur is not
// tokenised by segments but is the constant zero chunk - literal 0, 63 matches of 258 and one of 129 at distance 1 - of
// DF_ZERO_CHUNK_BYTES bytes (the segment rule takes 214).
constexpr int DF_ZERO_CHUNK_BYTES = 112;

// the zero chunk, built with the emitter itself (host): `out` takes DF_ZERO_CHUNK_BYTES bytes
inline void df_zero_chunk(uint8_t *out) {
    unsigned buf[DF_ZERO_CHUNK_BYTES / 4] = {};
    DfEmit<1> em(buf, 0);
    em.put(2u, 3);                                       // BFINAL = 0, BTYPE = 01
    em.literal(0);
    for (int i = 0; i < 63; ++i) em.match(258);
    em.match(129);
    em.finish();                                         // end-of-block, the stored block's header and LEN are zeros
    for (int b = 0; b < DF_ZERO_CHUNK_BYTES; ++b) out[b] = (uint8_t)(buf[b >> 2] >> ((b & 3) * 8));
    out[DF_ZERO_CHUNK_BYTES - 2] = out[DF_ZERO_CHUNK_BYTES - 1] = 0xFF;
}
