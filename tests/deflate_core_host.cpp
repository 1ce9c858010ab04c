// deflate_core_host.cpp - csrc/deflate_core.h compiled for the host (tests/test_deflate_core_host_cpu.py builds and runs it).
//   deflate_core_host bytes1 | bytes2            stdin: the file bytes of a map of 1- / 2-byte elements
//   deflate_core_host mask1 | mask2 <label>      stdin: a map of 1- / 2-byte labels; encoded is the mask of <label>
// stdout: the CRC-32 of the encoded bytes (4 bytes, little endian), then the fragment.  A chunk is encoded as a wave does
// it - count, place the lanes' bits, emit - with the lanes run one after the other and the plain `|=` of DfEmit.
#include "../fast-nnunet_amd/csrc/deflate_core.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint32_t g_tab[256];
static const DfTables g_t;
static const uint32_t g_x_chunk = df_xpow8(DF_CHUNK, g_t.x2k);

// one chunk of `len` bytes, rd(lane) the reader of the lane's segment: its bytes behind `out` -> its CRC-32
template <int DIST, class Rd> static uint32_t chunk(Rd rd, int len, std::vector<uint8_t> &out) {
    auto seg_len = [&](int lane) { const int l = len - lane * DF_SEG; return l < 0 ? 0 : (l > DF_SEG ? DF_SEG : l); };
    unsigned first[DF_LANES], all = 0;
    uint32_t crc = 0;
    for (int lane = 0; lane < DF_LANES; ++lane) {
        DfCount<DIST> cnt{g_tab};
        df_walk<DIST>(rd(lane), seg_len(lane), cnt);
        first[lane] = lane ? 3 + all : 0;
        all += cnt.bits;
        crc = df_crc_append(crc, ~cnt.crc, (unsigned long long)seg_len(lane), g_t.x2k, g_x_chunk);
    }
    const unsigned nbytes = df_chunk_bytes(all);
    std::vector<unsigned> buf(nbytes / 4 + 1, 0u);
    for (int lane = 0; lane < DF_LANES; ++lane) {
        DfEmit<DIST> em(buf.data(), first[lane]);
        if (lane == 0) em.put(2u, 3);
        df_walk<DIST>(rd(lane), seg_len(lane), em);
        em.finish();
    }
    for (unsigned b = 0; b < nbytes; ++b) out.push_back(b + 2 < nbytes ? (uint8_t)(buf[b >> 2] >> ((b & 3) * 8)) : (uint8_t)0xFF);
    return crc;
}

int main(int argc, char **argv) {
    if (argc < 2 || strlen(argv[1]) < 5 || (argv[1][0] == 'm' && argc < 3)) return 2;
    const bool mask = argv[1][0] == 'm';
    const int E = argv[1][strlen(argv[1]) - 1] - '0', W = mask ? E : 1;   // W: the bytes of one unit of a chunk's DF_CHUNK
    const unsigned label = mask ? (unsigned)strtoul(argv[2], nullptr, 10) : 0u;
    for (unsigned v = 0; v < 256; ++v) {
        uint32_t t = v;
        for (int i = 0; i < 8; ++i) t = (t >> 1) ^ ((t & 1) ? DF_POLY : 0u);
        g_tab[v] = t;
    }
    uint32_t zero_crc = 0xFFFFFFFFu;
    for (int i = 0; i < DF_CHUNK; ++i) zero_crc = g_tab[zero_crc & 255u] ^ (zero_crc >> 8);
    zero_crc = ~zero_crc;
    std::vector<uint8_t> data, out;
    for (int ch; (ch = getchar()) != EOF;) data.push_back((uint8_t)ch);
    const long long n = (long long)data.size() / W;
    uint32_t crc = 0;
    for (long long c = 0; c * DF_CHUNK < n; ++c) {
        const int len = n - c * DF_CHUNK < DF_CHUNK ? (int)(n - c * DF_CHUNK) : DF_CHUNK;
        std::vector<unsigned> in(DF_CHUNK * W / 4, 0u);           // the chunk as the kernels hold it: dwords, segment after segment
        memcpy(in.data(), data.data() + c * DF_CHUNK * W, (size_t)len * W);
        const unsigned *seg = in.data();
        bool occurs = false;
        for (int i = 0; mask && i < len; ++i) occurs |= ((seg[i * E / 4] >> (i * E % 4 * 8)) & (E == 1 ? 255u : 0xFFFFu)) == label;
        uint32_t ccrc = zero_crc;
        if (mask && len == DF_CHUNK && !occurs) {
            out.resize(out.size() + DF_ZERO_CHUNK_BYTES);
            df_zero_chunk(out.data() + out.size() - DF_ZERO_CHUNK_BYTES);
        } else if (mask && E == 1) ccrc = chunk<1>([&](int l) { return DfMask<1>{seg + l * DF_SEG / 4, label}; }, len, out);
        else if (mask) ccrc = chunk<1>([&](int l) { return DfMask<2>{seg + l * DF_SEG / 2, label}; }, len, out);
        else if (E == 1) ccrc = chunk<1>([&](int l) { return DfBytes{seg + l * DF_SEG / 4}; }, len, out);
        else ccrc = chunk<2>([&](int l) { return DfBytes{seg + l * DF_SEG / 4}; }, len, out);
        crc = df_crc_append(crc, ccrc, (unsigned long long)len, g_t.x2k, g_x_chunk);
    }
    const uint8_t head[4] = {(uint8_t)crc, (uint8_t)(crc >> 8), (uint8_t)(crc >> 16), (uint8_t)(crc >> 24)};
    fwrite(head, 1, 4, stdout);
    if (!out.empty()) fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
