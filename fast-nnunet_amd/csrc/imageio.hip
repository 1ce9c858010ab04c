// imageio.hip - the voxels of an image file as they lie in the file -> the float32 tensor the preprocessing reads, gfx950.
//
//   fnn_decode_voxels   n_vox elements of a NIfTI datatype (uint8 / int8 / int16 / uint16 / int32 / uint32 / float32 /
//                       float64, either byte order) -> float32, with the file's slope and intercept applied in float64.
//
// The value rule is what the reference's NibabelIO.read_images ends with (nibabel's get_fdata() in float64, then
// np.vstack(..., dtype=float32, casting='unsafe')): without scaling one conversion, round to nearest even; with scaling
// (float)((double)v * slope + inter), the product and the sum each rounded to float64 - never contracted into an FMA
// (the pragma below keeps the plain * and + of this file apart whatever -ffp-contract the build passes; hip's __dmul_rn /
// __dadd_rn are inline functions of a header compiled with the build's default, and the compiler does fuse them after
// inlining), the multiply skipped for slope == 1 and the add for inter == 0.
//
// One pass, bound by HBM.  A body thread owns V = max(4, 16 / sizeof(T)) consecutive elements whose float32 results start
// on a 16-byte boundary of `out`: 16-byte stores, and aligned 16-byte loads of the input.  `out` is only 4-byte aligned
// (channel c of a [C, ...] tensor starts c * n_vox floats in), so the body starts `head` (0..3) elements in; its input then
// starts head * sizeof(T) bytes past a 16-byte boundary and a thread reads one aligned chunk more and shifts (the extra
// chunk is its neighbour's first: the same cache line, no HBM traffic).  The elements before the body and those behind
// its last whole group whose chunks lie inside the input (`edge` elements, < 2 V + 4) go one per thread through the
// scalar path of the same launch.  Nothing is read outside raw[0, n_vox * sizeof(T)) or written outside out[0, n_vox).
#include "fnn_device.h"
#include "../../include/fnn.h"
#include <climits>
#include <cstdint>
#include <cstring>

#pragma clang fp contract(off)

namespace {

constexpr int DEC_THREADS = 256;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct DecodeArgs {
    const void *raw;             // 16-byte aligned
    float *out;                  // 4-byte aligned; out + head is 16-byte aligned
    long long n_vox;
    long long n_body;            // body threads (groups of V elements)
    int head;                    // elements before the body (0..3)
    int byteswap, scale, mul, add;
    double slope, inter;
};

template <typename T> static __device__ __forceinline__ T swap_bytes(T v) {
    if constexpr (sizeof(T) == 2) {
        const uint16_t u = __builtin_bit_cast(uint16_t, v);
        return __builtin_bit_cast(T, (uint16_t)__builtin_bswap16(u));
    } else if constexpr (sizeof(T) == 4) {
        return __builtin_bit_cast(T, __builtin_bswap32(__builtin_bit_cast(uint32_t, v)));
    } else if constexpr (sizeof(T) == 8) {
        return __builtin_bit_cast(T, __builtin_bswap64(__builtin_bit_cast(uint64_t, v)));
    } else {
        return v;
    }
}

template <typename T> static __device__ __forceinline__ float decode_one(T v, const DecodeArgs &a) {
    if (a.byteswap) v = swap_bytes<T>(v);
    if (!a.scale) return (float)v;                       // one rounding, to nearest even (identity for float32)
    double d = (double)v;
    if (a.mul) d = d * a.slope;                          // (contraction is off in this file: two IEEE operations)
    if (a.add) d = d + a.inter;
    return (float)d;
}

// dwords WS .. WS + ND - 1 of w shifted down by `bs` bits (0, 8, 16, 24) into d
template <int WS, int ND> static __device__ __forceinline__ void shift_dwords(const unsigned (&w)[ND + 4], int bs, unsigned (&d)[ND]) {
#pragma unroll
    for (int j = 0; j < ND; ++j)
        d[j] = (unsigned)((((unsigned long long)w[j + WS + 1] << 32) | w[j + WS]) >> bs);
}

template <typename T>
__global__ __launch_bounds__(DEC_THREADS) void decode_voxels_kernel(DecodeArgs a) {
    constexpr int SZ = sizeof(T), V = SZ >= 4 ? 4 : 16 / SZ, NC = V * SZ / 16, ND = 4 * NC;
    const long long gid = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (gid < a.n_body) {
        const long long e0 = a.head + gid * V;                       // first element of the group
        const int hb = a.head * SZ;                                  // bytes the body's input starts past raw
        const int s = hb & 15;                                       // ... past a 16-byte boundary (the same for every group)
        const u32x4 *src = (const u32x4 *)a.raw + (hb >> 4) + gid * NC;
        unsigned w[ND + 4], d[ND];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const u32x4 q = src[c];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[4 * c + k] = q[k];
        }
        if (s) {                                                     // uniform: n_body only counts groups whose extra chunk exists
            const u32x4 q = src[NC];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[ND + k] = q[k];
            const int bs = (s & 3) * 8;
            switch (s >> 2) {
            case 0: shift_dwords<0, ND>(w, bs, d); break;
            case 1: shift_dwords<1, ND>(w, bs, d); break;
            case 2: shift_dwords<2, ND>(w, bs, d); break;
            default: shift_dwords<3, ND>(w, bs, d); break;
            }
        } else {
#pragma unroll
            for (int j = 0; j < ND; ++j) d[j] = w[j];
        }
        T v[V];
        __builtin_memcpy(v, d, sizeof(v));
#pragma unroll
        for (int q = 0; q < V / 4; ++q) {
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = decode_one<T>(v[4 * q + k], a);
            *(f32x4 *)(a.out + e0 + 4 * q) = o;
        }
        return;
    }
    // the edges: the `head` elements before the body, then everything behind it
    long long e = gid - a.n_body;
    if (e >= a.head) e += a.n_body * V;
    if (e < a.n_vox) a.out[e] = decode_one<T>(((const T *)a.raw)[e], a);
}

template <typename T> static hipError_t launch_decode(DecodeArgs a, int *rc, hipStream_t st) {
    constexpr long long SZ = sizeof(T), V = SZ >= 4 ? 4 : 16 / SZ, NC = V * SZ / 16;
    const long long hb = a.head * SZ, chunks = a.n_vox * SZ / 16;    // whole 16-byte chunks inside the input
    // group g reads chunks (hb >> 4) + g NC .. + NC - 1, and one more when the body's input is shifted
    const long long need = NC + ((hb & 15) ? 1 : 0);
    long long groups = (chunks - (hb >> 4) - need) / NC + 1;
    if (chunks - (hb >> 4) < need) groups = 0;
    const long long fit = (a.n_vox - a.head) / V;                    // ... and writes V whole elements
    a.n_body = groups < fit ? groups : fit;
    if (a.n_body < 0) a.n_body = 0;
    const long long threads = a.n_body + (a.n_vox - a.n_body * V);
    const long long blocks = (threads + DEC_THREADS - 1) / DEC_THREADS;
    if (blocks > INT_MAX) { *rc = FNN_E_UNSUPPORTED; return hipSuccess; }
    hipLaunchKernelGGL(decode_voxels_kernel<T>, dim3((unsigned)blocks), dim3(DEC_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace

extern "C" int fnn_decode_voxels(const void *raw, int nifti_datatype, int byteswap, int64_t n_vox, int scale, double slope,
                                 double inter, float *out, void *stream) {
    if (!raw || !out) return fnn_fail(FNN_E_INVALID, "NULL argument");
    if (n_vox < 0) return fnn_fail(FNN_E_INVALID, "negative n_vox");
    if ((uintptr_t)raw % 16) return fnn_fail(FNN_E_INVALID, "fnn_decode_voxels: raw must be 16-byte aligned");
    if ((uintptr_t)out % 4) return fnn_fail(FNN_E_INVALID, "fnn_decode_voxels: out must be 4-byte aligned");
    switch (nifti_datatype) {
    case 2: case 256: case 4: case 512: case 8: case 768: case 16: case 64: break;
    default: return fnn_fail(FNN_E_UNSUPPORTED, "fnn_decode_voxels: NIfTI datatype not served (uint8, int8, int16, uint16, int32, "
                                                "uint32, float32 and float64 are)");
    }
    if (n_vox == 0) return FNN_OK;
    if (!fnn_dev_ptr(raw) || !fnn_dev_ptr(out)) return fnn_fail(FNN_E_INVALID, "fnn_decode_voxels needs device pointers (no CPU path)");
    DecodeArgs a{};
    a.raw = raw; a.out = out; a.n_vox = n_vox;
    a.head = (int)(((16 - ((uintptr_t)out & 15)) & 15) / 4);
    if (a.head > n_vox) a.head = (int)n_vox;
    a.byteswap = byteswap != 0; a.scale = scale != 0;
    a.slope = slope; a.inter = inter;
    a.mul = slope != 1.0; a.add = inter != 0.0;
    hipStream_t st = (hipStream_t)stream;
    int rc = FNN_OK;
    hipError_t r = hipSuccess;
    switch (nifti_datatype) {
    case 2: r = launch_decode<uint8_t>(a, &rc, st); break;
    case 256: r = launch_decode<int8_t>(a, &rc, st); break;
    case 4: r = launch_decode<int16_t>(a, &rc, st); break;
    case 512: r = launch_decode<uint16_t>(a, &rc, st); break;
    case 8: r = launch_decode<int32_t>(a, &rc, st); break;
    case 768: r = launch_decode<uint32_t>(a, &rc, st); break;
    case 16: r = launch_decode<float>(a, &rc, st); break;
    default: r = launch_decode<double>(a, &rc, st); break;
    }
    if (rc != FNN_OK) return fnn_fail(rc, "fnn_decode_voxels: too many voxels for one launch");
    if (r != hipSuccess) return fnn_fail(FNN_E_HIP, hipGetErrorString(r));
    return FNN_OK;
}
