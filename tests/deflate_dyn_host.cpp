// deflate_dyn_host.cpp - csrc/deflate_dyn_core.h compiled for the host (tests/test_deflate_dyn_host_cpu.py builds and runs it).
//   deflate_dyn_host bytes1 | bytes2     stdin: the file bytes of a map of 1- / 2-byte elements
//                                        stdout: the CRC-32 (4 bytes, little endian), the chunks that took their own
//                                        tables (4 bytes), then the fragment
//   deflate_dyn_host lengths <limit>     stdin: frequencies, 4 bytes each (at most 286); stdout: df_code_lengths' lengths
// A chunk is encoded as a wave does it - walk, tables, choice, walk, emit - with the lanes run one after the other
// (DfSerial) and the plain `|=` of DfEmit.
#include "../fast-nnunet_amd/csrc/deflate_dyn_core.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint32_t g_tab[256];
static const DfTables g_t;
static const uint32_t g_x_chunk = df_xpow8(DF_CHUNK, g_t.x2k);

static int seg_len(int len, int lane) { const int l = len - lane * DF_SEG; return l < 0 ? 0 : (l > DF_SEG ? DF_SEG : l); }

// one chunk of `len` bytes at `seg` (dwords, segment after segment): its bytes behind `out` -> its CRC-32
template <int DIST> static uint32_t chunk(const unsigned *seg, int len, std::vector<uint8_t> &out, unsigned &dynamic_chunks) {
    static DfDynWork k;
    memset(&k, 0xA5, sizeof(k));                                  // nothing is read that was not written
    for (int s = 0; s < DF_NLIT; ++s) k.freq[s] = 0;
    unsigned fixed[DF_LANES], bits[DF_LANES], all_fixed = 0, all = 0;
    uint32_t crc = 0;
    for (int lane = 0; lane < DF_LANES; ++lane) {
        DfDynCount<DIST> cnt{DfCount<DIST>{g_tab}, k.freq};
        df_walk<DIST>(DfBytes{seg + lane * DF_SEG / 4}, seg_len(len, lane), cnt);
        cnt.finish();
        all_fixed += fixed[lane] = cnt.fixed.bits;
        crc = df_crc_append(crc, ~cnt.fixed.crc, (unsigned long long)seg_len(len, lane), g_t.x2k, g_x_chunk);
    }
    ++k.freq[256];
    df_dyn_tables(k, DfSerial{});
    const unsigned dyn_block = (unsigned)k.hdr_bits + df_dyn_token_bits(k, DfSerial{}), fixed_block = 3 + all_fixed + 7;
    const bool dynamic = dyn_block < fixed_block;
    const unsigned nbytes = df_block_chunk_bytes(dynamic ? dyn_block : fixed_block);
    std::vector<unsigned> buf(nbytes / 4 + 2, 0u);
    if (dynamic) {
        ++dynamic_chunks;
        uint32_t packed[DF_LEN_DWORDS], code[DF_NLIT_PAD], next[16];
        uint8_t lens[DF_NLIT_PAD];
        for (int d = 0; d < DF_LEN_DWORDS; ++d) packed[d] = df_pack_lengths(k.len, d);      // ... as the emit pass reads them back
        for (int s = 0; s < DF_NLIT_PAD; ++s) lens[s] = (uint8_t)((packed[s >> 3] >> (4 * (s & 7))) & 15u);
        df_canonical(lens, DF_NLIT, code, next, DfSerial{});
        for (int d = 0; d * 32 < k.hdr_bits; ++d) buf[d] |= k.hdr[d];
        for (int lane = 0; lane < DF_LANES; ++lane) {
            DfDynBits cost{lens};
            df_walk<DIST>(DfBytes{seg + lane * DF_SEG / 4}, seg_len(len, lane), cost);
            bits[lane] = cost.bits;
        }
        unsigned first = (unsigned)k.hdr_bits;
        for (int lane = 0; lane < DF_LANES; ++lane) {
            DfDynEmit<DIST> em{DfEmit<DIST>(buf.data(), first), code};
            df_walk<DIST>(DfBytes{seg + lane * DF_SEG / 4}, seg_len(len, lane), em);
            if (lane == DF_LANES - 1) em.symbol(256);
            em.em.finish();
            first += bits[lane];
        }
        all = first;
        if (all + (lens[256]) != dyn_block) abort();            // the histogram's total is the walks'
    } else {
        unsigned first = 0;
        for (int lane = 0; lane < DF_LANES; ++lane) {
            DfEmit<DIST> em(buf.data(), lane ? 3 + first : 0);
            if (lane == 0) em.put(2u, 3);
            df_walk<DIST>(DfBytes{seg + lane * DF_SEG / 4}, seg_len(len, lane), em);
            em.finish();
            first += fixed[lane];
        }
    }
    for (unsigned b = 0; b < nbytes; ++b) out.push_back(b + 2 < nbytes ? (uint8_t)(buf[b >> 2] >> ((b & 3) * 8)) : (uint8_t)0xFF);
    return crc;
}

static void put32(uint32_t v) {
    const uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
    fwrite(b, 1, 4, stdout);
}

int main(int argc, char **argv) {
    if (argc < 2 || strlen(argv[1]) < 6) return 2;
    std::vector<uint8_t> data, out;
    for (int ch; (ch = getchar()) != EOF;) data.push_back((uint8_t)ch);
    if (argv[1][0] == 'l') {
        if (argc < 3) return 2;
        const int limit = atoi(argv[2]), n = (int)(data.size() / 4);
        if (n > DF_NLIT || limit < 1 || limit > 15) return 2;
        static DfHuffWork k;
        std::vector<uint32_t> freq((size_t)n + 1);
        std::vector<uint8_t> len((size_t)n + 1);
        memcpy(freq.data(), data.data(), (size_t)n * 4);
        df_code_lengths(freq.data(), n, limit, len.data(), k, DfSerial{});
        fwrite(len.data(), 1, (size_t)n, stdout);
        return 0;
    }
    const int E = argv[1][strlen(argv[1]) - 1] - '0';
    for (unsigned v = 0; v < 256; ++v) {
        uint32_t t = v;
        for (int i = 0; i < 8; ++i) t = (t >> 1) ^ ((t & 1) ? DF_POLY : 0u);
        g_tab[v] = t;
    }
    const long long n = (long long)data.size();
    uint32_t crc = 0;
    unsigned dynamic_chunks = 0;
    for (long long c = 0; c * DF_CHUNK < n; ++c) {
        const int len = n - c * DF_CHUNK < DF_CHUNK ? (int)(n - c * DF_CHUNK) : DF_CHUNK;
        std::vector<unsigned> in(DF_CHUNK / 4, 0u);               // the chunk as the kernels hold it: dwords, segment after segment
        memcpy(in.data(), data.data() + c * DF_CHUNK, (size_t)len);
        const uint32_t ccrc = E == 1 ? chunk<1>(in.data(), len, out, dynamic_chunks) : chunk<2>(in.data(), len, out, dynamic_chunks);
        crc = df_crc_append(crc, ccrc, (unsigned long long)len, g_t.x2k, g_x_chunk);
    }
    put32(crc);
    put32(dynamic_chunks);
    if (!out.empty()) fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
