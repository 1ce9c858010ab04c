// inflate_dyn_wave.h - a dynamic block's tables as one wave of 64 lanes keeps them (InfWaveStore, the `Store` of
// inflate_dyn_core.h), device only: built by the lanes in LDS and decoded canonically across them.  csrc/inflate_dyn.hip
// describes how; its kernels and those of csrc/inflate_any.hip decode with it.  The workgroup is the one wave: the barriers
// in here order that wave's LDS accesses alone.
#pragma once
#include "inflate_dyn_core.h"
#include "inflate_wave.h"

constexpr int INF_LIST_LIT = 288, INF_LIST_SMALL = 32;           // the sorted lists' entries, for 286, 30 and 19 symbols
constexpr int INF_TABLE_BYTES = 2 * (INF_DYN_SEQ + INF_LIST_LIT + 2 * INF_LIST_SMALL);
static_assert(INF_TABLE_BYTES == 1408, "the figure in the comment above");

// what lane l keeps of one code, for the length l = 1 .. 15 (0 in every other lane: its limit admits no pattern)
struct InfLaneCode {
    int count = 0;
    int first = 0;                                               // the first code of the length, left-justified to 15 bits
    int limit = 0;                                               // behind its last code, left-justified
    int place = 0;                                               // of its first symbol in the sorted list
};

struct InfWaveStore {
    uint16_t *s_seq;                                             // INF_DYN_SEQ entries: length | rank << 4
    uint16_t *s_sorted;                                          // the lists: literal / length, distance, code-length
    int lane;
    InfLaneCode cl, lit, dist;
    __device__ __forceinline__ InfWaveStore(uint16_t *tables, int lane_) : s_seq(tables), s_sorted(tables + INF_DYN_SEQ), lane(lane_) {}

    template <int W> __device__ __forceinline__ InfLaneCode &code() { return W == INF_CODE_CL ? cl : W == INF_CODE_LIT ? lit : dist; }
    template <int W> __device__ __forceinline__ const InfLaneCode &code() const { return W == INF_CODE_CL ? cl : W == INF_CODE_LIT ? lit : dist; }
    template <int W> __device__ __forceinline__ uint16_t *list() const {
        return s_sorted + (W == INF_CODE_LIT ? 0 : W == INF_CODE_DIST ? INF_LIST_LIT : INF_LIST_LIT + INF_LIST_SMALL);
    }
    // a place in code W's list, whatever `at` is: clamped to the 288 entries, or masked to the 32
    template <int W> static __device__ __forceinline__ int bounded(int at) {
        return W == INF_CODE_LIT ? (int)min((unsigned)at, (unsigned)INF_LIST_LIT - 1u) : at & (INF_LIST_SMALL - 1);
    }
    template <int W> static constexpr int rounds() { return W == INF_CODE_LIT ? 5 : 1; }     // 64 symbols a round: 286, 30, 19

    // i < INF_DYN_SEQ and i + rep <= INF_DYN_SEQ by the rule
    __device__ __forceinline__ void set_len(int i, int len) {
        if (lane == 0) s_seq[i] = (uint16_t)len;
    }
    __device__ __forceinline__ void set_run(int i, int rep, int len) {
        for (int j = lane; j < rep; j += DF_LANES) s_seq[i + j] = (uint16_t)len;
    }

    template <int W> __device__ __forceinline__ void count(int lo, int n) {
        InfLaneCode &c = code<W>();
        c.count = 0;
        const unsigned long long below = (1ull << lane) - 1ull;
        __syncthreads();                                         // the lengths are all there
#pragma unroll
        for (int k = 0; k < rounds<W>(); ++k) {
            const int s = k * DF_LANES + lane;
            const int len = s < n ? s_seq[lo + s] & 15 : 0;
            int rank = 0;
#pragma unroll
            for (int l = 1; l <= 15; ++l) {
                const unsigned long long has = __ballot(len == l);
                const int before = __builtin_amdgcn_readlane(c.count, l);
                if (len == l) rank = before + __popcll(has & below);
                if (lane == l) c.count += __popcll(has);
            }
            if (s < n) s_seq[lo + s] = (uint16_t)(len | rank << 4);
        }
    }
    template <int W> __device__ __forceinline__ int count_of(int l) const { return __builtin_amdgcn_readlane(code<W>().count, l); }
    template <int W> __device__ __forceinline__ void set_code(int l, int first, int count, int place) {
        InfLaneCode &c = code<W>();
        if (lane == l) {
            c.first = first << (15 - l);
            c.limit = (first + count) << (15 - l);
            c.place = place;
        }
    }
    template <int W> __device__ __forceinline__ void sort(int lo, int n) {
        const InfLaneCode &c = code<W>();
#pragma unroll
        for (int k = 0; k < rounds<W>(); ++k) {
            const int s = k * DF_LANES + lane;
            const int e = s < n ? s_seq[lo + s] : 0;
            const int at = __shfl(c.place, e & 15) + (e >> 4);   // (lane 0, for no code: its place is 0, and nothing is stored)
            if (e & 15) list<W>()[bounded<W>(at)] = (uint16_t)s;
        }
        __syncthreads();                                         // the list is complete before the first lookup
    }
    template <int W> __device__ __forceinline__ int symbol(unsigned v, int &n) const {
        const InfLaneCode &c = code<W>();
        const int bits = (int)(__builtin_bitreverse32(v) >> 17);                 // the 15 bits as a code, first bit highest
        const unsigned long long fits = __ballot(bits < c.limit);
        if (fits == 0) {
            n = 1;
            return -1;
        }
        const int l = __builtin_ctzll(fits);                                     // 1 .. 15: only those lanes have a limit
        n = l;
        const int first = __builtin_amdgcn_readlane(c.first, l), place = __builtin_amdgcn_readlane(c.place, l);
        const int at = place + ((bits - first) >> (15 - l));
        return __builtin_amdgcn_readfirstlane((int)list<W>()[bounded<W>(at)]);
    }
};
