// reorient.hip - flip and permute the axes of a C-order 3-D array of 1-, 2- or 4-byte elements on the device, gfx950.
//
//   fnn_reorient   out[i0, i1, i2] = in[j],  j[src_axis[d]] = flip[d] ? shape_in[src_axis[d]] - 1 - i_d : i_d
//
// What the reorienting reader-writer needs twice per case: the decoded float32 voxels of a file into the RAS frame, and the
// uint8 / uint16 labels back into the file's frame.  Pure data movement: numpy's flip and transpose, bit for bit.
//
// Every output axis d walks the input with a signed element stride st[d] (+-1 for the output axis that is the input's fastest
// one) from the input element `base` of output element (0, 0, 0); both kernels only differ in how they visit the output.
//
//   reorient_rows_kernel<SZ>        src_axis[2] == 2: rows stay rows.  A thread owns one 16-byte aligned chunk of the output
//     (16 / SZ elements).  When the chunk lies inside one output row its source is one contiguous run, read as whole aligned
//     dwords (an element-aligned run of 1- or 2-byte elements through one dword more and a funnel shift - only where those
//     dwords lie inside the input), reversed in registers when the row is flipped, and stored with one 16-byte store.  Chunks
//     that straddle a row end, the first and last partial chunks of `out`, and runs whose dwords would reach outside the input
//     go element by element.
//
//   reorient_transpose_kernel<SZ>   src_axis[2] != 2: a T x T = 64 x 64 element tile of the plane spanned by the input's
//     fastest axis (output axis q) and the output's fastest axis goes through LDS.  Load: a wave reads 64 consecutive input
//     elements (one run along the input's fastest axis) per instruction, a lane packs the 4 / SZ elements of consecutive output
//     columns into one dword and writes it to tile[x][kd].  Store: W = 64 SZ / 4 lanes per output row own the aligned dwords
//     of its run of <= 64 elements (the row starts at any element, so a lane combines two tile dwords with a funnel shift);
//     whole dwords are stored as dwords, the elements before the first and behind the last whole dword one by one.
//     LDS banks (32 dwords for ds_write_b32 / ds_read_b32, conflicts within a half wave): 4-byte elements pitch 65 and
//     2-byte elements pitch 33 - odd, so the 32 rows a half wave writes fall on 32 banks, and a half wave reads consecutive
//     dwords of one row; 1-byte elements have 16 dwords per row: pitch 16 with the column XOR-ed by (x >> 1) & 15, so that
//     the 32 rows of a write (bank 16 (x & 1) + (kd ^ (x >> 1))) and the two rows x, x + 1 (x even) of a read each cover
//     all 32 banks once.
//
// Nothing is read outside in[0, n) or written outside out[0, n).  Neither kernel keeps scratch.
#include "host_call.h"
#include <climits>
#include <cstdint>

namespace {

constexpr int RO_THREADS = 256;
constexpr int RO_TILE = 64;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int SZ> struct elem_of;
template <> struct elem_of<1> { typedef uint8_t type; };
template <> struct elem_of<2> { typedef uint16_t type; };
template <> struct elem_of<4> { typedef uint32_t type; };

struct ReorientArgs {
    const void *in;
    void *out;
    long long n;                     // elements
    long long o1, o2;                // output extents of axes 1 and 2
    long long st0, st1, st2;         // signed input stride (elements) of each output axis
    long long base;                  // input element of output element (0, 0, 0)
    int small;                       // n < 2^31: 32-bit divisions
    // rows
    int mis;                         // elements between the 16-byte boundary below `out` and `out`
    long long chunks;                // 16-byte chunks that hold output elements
    // transpose: q = the output axis (0 or 1) that is the input's fastest one, r the other
    int q;
    long long oq, stq, str;          // extent and stride of q, stride of r
    long long tq, t2;                // tiles along q and along output axis 2
};

static __device__ __forceinline__ void divmod(long long v, long long d, int small, long long &quo, long long &rem) {
    if (small) {
        const unsigned a = (unsigned)v, b = (unsigned)d;
        quo = a / b;
        rem = a - (unsigned)quo * b;
    } else {
        quo = v / d;
        rem = v - quo * d;
    }
}

// the 16 bytes of the run that starts at element s of `in` (n elements) -> d; false when aligned dwords cannot serve it
template <int SZ>
static __device__ __forceinline__ bool load_run(const typename elem_of<SZ>::type *in, long long s, long long n, unsigned (&d)[4]) {
    const uintptr_t a = (uintptr_t)(in + s);
    const int al = SZ == 4 ? 0 : (int)(a & 3);
    if (al == 0) {
        if ((a & 15) == 0) {
            const u32x4 v = *(const u32x4 *)a;
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = v[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = ((const unsigned *)a)[k];
        }
        return true;
    }
    const uintptr_t lo = a - al;                                     // five dwords lo .. lo + 20 cover the run
    if (lo < (uintptr_t)in || lo + 20 > (uintptr_t)(in + n)) return false;
    unsigned w[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) w[k] = ((const unsigned *)lo)[k];
    const int bs = al * 8;
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = (unsigned)((((unsigned long long)w[k + 1] << 32) | w[k]) >> bs);
    return true;
}

// the 16 / SZ elements of d in reverse order
template <int SZ> static __device__ __forceinline__ void reverse_run(unsigned (&d)[4]) {
    unsigned t = d[0]; d[0] = d[3]; d[3] = t;
    t = d[1]; d[1] = d[2]; d[2] = t;
    if constexpr (SZ == 2) {
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = (d[k] >> 16) | (d[k] << 16);
    } else if constexpr (SZ == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = __builtin_bswap32(d[k]);
    }
}

template <int SZ>
__global__ __launch_bounds__(RO_THREADS) void reorient_rows_kernel(ReorientArgs a) {
    typedef typename elem_of<SZ>::type E;
    constexpr int V = 16 / SZ;
    const long long c = (long long)blockIdx.x * RO_THREADS + threadIdx.x;
    if (c >= a.chunks) return;
    const long long e0 = c * V - a.mis;                              // the chunk's first output element (< 0: before `out`)
    const E *in = (const E *)a.in;
    E *out = (E *)a.out;
    if (e0 >= 0 && e0 + V <= a.n) {
        long long row, x;
        divmod(e0, a.o2, a.small, row, x);
        if (x + V <= a.o2) {                                         // one row: one contiguous run of the input
            long long i0, i1;
            divmod(row, a.o1, a.small, i0, i1);
            const long long s = a.base + i0 * a.st0 + i1 * a.st1 + (a.st2 > 0 ? x : -(x + V - 1));
            unsigned d[4];
            if (load_run<SZ>(in, s, a.n, d)) {
                if (a.st2 < 0) reverse_run<SZ>(d);
                u32x4 v;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = d[k];
                *(u32x4 *)(out + e0) = v;
                return;
            }
        }
    }
    for (int j = 0; j < V; ++j) {
        const long long e = e0 + j;
        if (e < 0 || e >= a.n) continue;
        long long row, x, i0, i1;
        divmod(e, a.o2, a.small, row, x);
        divmod(row, a.o1, a.small, i0, i1);
        out[e] = in[a.base + i0 * a.st0 + i1 * a.st1 + x * a.st2];
    }
}

template <int SZ> static __device__ __forceinline__ int tile_index(int x, int kd) {
    constexpr int W = RO_TILE * SZ / 4;
    if constexpr (SZ == 1) return x * W + (kd ^ ((x >> 1) & (W - 1)));
    else return x * (W + 1) + kd;
}

template <int SZ>
__global__ __launch_bounds__(RO_THREADS) void reorient_transpose_kernel(ReorientArgs a) {
    typedef typename elem_of<SZ>::type E;
    constexpr int T = RO_TILE, V = 4 / SZ, W = T / V;                // V elements per dword, W dwords per tile row
    constexpr int PITCH = SZ == 1 ? W : W + 1;
    __shared__ unsigned tile[T * PITCH];
    long long blk = blockIdx.x;
    const long long tb = blk % a.t2;
    blk /= a.t2;
    const long long ta = blk % a.tq, ir = blk / a.tq;
    const long long a0 = ta * T, b0 = tb * T;                        // the tile's origin along q and along output axis 2
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const E *in = (const E *)a.in;
    E *out = (E *)a.out;
    {   // load: lane = position along the input's fastest axis, a wave per dword column
        const long long iq = a0 + lane;
        const long long src = a.base + ir * a.str + iq * a.stq;
        for (int kd = wave; kd < W; kd += RO_THREADS / 64) {
            unsigned d = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const long long i2 = b0 + kd * V + j;
                if (iq < a.oq && i2 < a.o2) d |= (unsigned)in[src + i2 * a.st2] << (j * SZ * 8);
            }
            tile[tile_index<SZ>(lane, kd)] = d;
        }
    }
    __syncthreads();
    const long long left = a.o2 - b0;
    const int n = left < T ? (int)left : T;                          // elements of every output run of this tile
    constexpr int RPW = 64 / W;                                      // output rows per wave and pass
    const int g = lane / W, lg = lane % W;
    for (int x = wave * RPW + g; x < T; x += (RO_THREADS / 64) * RPW) {
        const long long iq = a0 + x;
        if (iq >= a.oq) break;
        const long long row = a.q == 0 ? iq * a.o1 + ir : ir * a.o1 + iq;
        E *p = out + row * a.o2 + b0;                                // the run's first element
        const int mis = SZ == 4 ? 0 : (int)(((uintptr_t)p & 3) / SZ);   // elements behind the dword boundary below p
        for (int l = lg; l <= W; l += W) {                           // dword l of the run's span; lane 0 also takes the last, partial one
            if (l == W && (lg != 0 || mis == 0)) break;
            const int f = l * V - mis;                               // its first element within the run
            if (f >= n) break;
            unsigned d;
            if constexpr (SZ == 4) {
                d = tile[tile_index<SZ>(x, l)];
            } else {
                const unsigned hi = l < W ? tile[tile_index<SZ>(x, l)] : 0u;
                const unsigned lo = (mis && l > 0) ? tile[tile_index<SZ>(x, l - 1)] : 0u;
                d = (unsigned)((((unsigned long long)hi << 32) | lo) >> ((V - mis) * SZ * 8));
            }
            if (f >= 0 && f + V <= n) {
                *(unsigned *)(p + f) = d;
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j)
                    if (f + j >= 0 && f + j < n) p[f + j] = (E)(d >> (j * SZ * 8));
            }
        }
    }
}

template <int SZ> static hipError_t launch_reorient(const ReorientArgs &a, bool rows, long long blocks, hipStream_t st) {
    if (rows) hipLaunchKernelGGL(reorient_rows_kernel<SZ>, dim3((unsigned)blocks), dim3(RO_THREADS), 0, st, a);
    else hipLaunchKernelGGL(reorient_transpose_kernel<SZ>, dim3((unsigned)blocks), dim3(RO_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace

extern "C" int fnn_reorient(const void *in, int elem_bytes, const int64_t shape_in[3], const int32_t src_axis[3],
                            const int32_t flip[3], void *out, void *stream) {
    if (!in || !out || !shape_in || !src_axis || !flip) return fnn_fail(FNN_E_INVALID, "NULL argument");
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4)
        return fnn_fail(FNN_E_UNSUPPORTED, "fnn_reorient: elements of 1, 2 or 4 bytes are served");
    if (!fnn_is_perm(src_axis)) return fnn_fail(FNN_E_INVALID, "fnn_reorient: src_axis must be a permutation of 0, 1, 2");
    long long n = 1;
    for (int d = 0; d < 3; ++d) {
        if (shape_in[d] < 0) return fnn_fail(FNN_E_INVALID, "fnn_reorient: negative extent");
        if (__builtin_mul_overflow(n, (long long)shape_in[d], &n) || n > (LLONG_MAX >> 4))
            return fnn_fail(FNN_E_UNSUPPORTED, "fnn_reorient: too many elements for one launch");
    }
    if ((uintptr_t)in % elem_bytes || (uintptr_t)out % elem_bytes)
        return fnn_fail(FNN_E_INVALID, "fnn_reorient: in and out must be aligned to the element size");
    if (n == 0) return FNN_OK;
    const uintptr_t bytes = (uintptr_t)n * elem_bytes, ia = (uintptr_t)in, oa = (uintptr_t)out;
    if (ia < oa + bytes && oa < ia + bytes) return fnn_fail(FNN_E_INVALID, "fnn_reorient: in and out overlap");

    const long long in_stride[3] = {(long long)shape_in[1] * shape_in[2], (long long)shape_in[2], 1};
    long long o[3], st[3], base = 0;
    for (int d = 0; d < 3; ++d) {
        o[d] = shape_in[src_axis[d]];
        st[d] = in_stride[src_axis[d]];
        if (flip[d]) { base += (o[d] - 1) * st[d]; st[d] = -st[d]; }
    }
    ReorientArgs a{};
    a.in = in; a.out = out; a.n = n;
    a.o1 = o[1]; a.o2 = o[2];
    a.st0 = st[0]; a.st1 = st[1]; a.st2 = st[2];
    a.base = base;
    a.small = n < (1LL << 31);
    const bool rows = src_axis[2] == 2;
    if (!rows) {
        a.q = src_axis[0] == 2 ? 0 : 1;
        a.oq = o[a.q]; a.stq = st[a.q]; a.str = st[1 - a.q];
        a.tq = (a.oq + RO_TILE - 1) / RO_TILE;
        a.t2 = (a.o2 + RO_TILE - 1) / RO_TILE;
    }
    long long blocks;
    if (rows) {
        const long long v = 16 / elem_bytes;
        a.mis = (int)(((uintptr_t)out & 15) / elem_bytes);
        a.chunks = (a.mis + n + v - 1) / v;
        blocks = (a.chunks + RO_THREADS - 1) / RO_THREADS;
    } else {
        const long long outer = o[1 - a.q];
        blocks = a.tq * a.t2 > INT_MAX / outer ? (long long)INT_MAX + 1 : a.tq * a.t2 * outer;
    }
    if (blocks > INT_MAX) return fnn_fail(FNN_E_UNSUPPORTED, "fnn_reorient: too many elements for one launch");
    if (int rc = fnn_need_dev("fnn_reorient", {in, out})) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipError_t r;
    switch (elem_bytes) {
    case 1: r = launch_reorient<1>(a, rows, blocks, s); break;
    case 2: r = launch_reorient<2>(a, rows, blocks, s); break;
    default: r = launch_reorient<4>(a, rows, blocks, s); break;
    }
    if (r != hipSuccess) return fnn_fail(FNN_E_HIP, hipGetErrorString(r));
    return FNN_OK;
}
