// imageio.hip - the voxels of an image file as they lie in the file -> the float32 tensor the preprocessing reads, gfx950.
//
//   fnn_decode_voxels   n_vox elements of a NIfTI datatype (uint8 / int8 / int16 / uint16 / int32 / uint32 / float32 /
//                       float64, either byte order) -> float32, with the file's slope and intercept applied in float64.
//
//   fnn_decode_labels   the same voxels of a label file -> uint8 / uint16 labels, every voxel judged by the float32 that
//                       fnn_decode_voxels stores for it; what is no label stores 0 and raises a flag (see below).
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
#include "host_call.h"
#include <climits>
#include <cstdint>
#include <cstring>
#include <type_traits>

#pragma clang fp contract(off)

namespace {

constexpr int DEC_THREADS = 256;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct DecodeArgs {
    const void *raw;             // 16-byte aligned
    float *out;                  // 4-byte aligned; out + head is 16-byte aligned (unused by the label kernel: LabelArgs::out)
    long long n_vox;
    long long n_body;            // body threads (groups of V elements)
    int head;                    // elements before the body: 0..3 for float32 out, 0..15 for labels (16 / OB - 1)
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

// the elements one body thread owns: V of them, NC aligned 16-byte chunks of input (ND dwords)
template <typename T> struct Group {
    static constexpr int SZ = sizeof(T), V = SZ >= 4 ? 4 : 16 / SZ, NC = V * SZ / 16, ND = 4 * NC;
};

// group `gid` of the body, whose input starts a.head elements (any number of bytes past a 16-byte boundary) behind raw
template <typename T> static __device__ __forceinline__ void load_group(const DecodeArgs &a, long long gid, T (&v)[Group<T>::V]) {
    constexpr int SZ = Group<T>::SZ, NC = Group<T>::NC, ND = Group<T>::ND;
    const int hb = a.head * SZ;                                      // bytes the body's input starts past raw
    const int s = hb & 15;                                           // ... past a 16-byte boundary (the same for every group)
    const u32x4 *src = (const u32x4 *)a.raw + (hb >> 4) + gid * NC;
    unsigned w[ND + 4], d[ND];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const u32x4 q = src[c];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[4 * c + k] = q[k];
    }
    if (s) {                                                         // uniform: n_body only counts groups whose extra chunk exists
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
    __builtin_memcpy(v, d, sizeof(v));
}

// the body groups of a launch: those whose chunks lie inside the input and whose V elements lie inside the output
template <typename T> static long long body_groups(long long n_vox, int head) {
    constexpr long long SZ = Group<T>::SZ, V = Group<T>::V, NC = Group<T>::NC;
    const long long hb = head * SZ, chunks = n_vox * SZ / 16;        // whole 16-byte chunks inside the input
    // group g reads chunks (hb >> 4) + g NC .. + NC - 1, and one more when the body's input is shifted
    const long long need = NC + ((hb & 15) ? 1 : 0);
    long long groups = (chunks - (hb >> 4) - need) / NC + 1;
    if (chunks - (hb >> 4) < need) groups = 0;
    const long long fit = (n_vox - head) / V;                        // ... and writes V whole elements
    const long long n_body = groups < fit ? groups : fit;
    return n_body < 0 ? 0 : n_body;
}

template <typename T>
__global__ __launch_bounds__(DEC_THREADS) void decode_voxels_kernel(DecodeArgs a) {
    constexpr int V = Group<T>::V;
    const long long gid = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (gid < a.n_body) {
        const long long e0 = a.head + gid * V;                       // first element of the group
        T v[V];
        load_group<T>(a, gid, v);
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
    constexpr long long V = Group<T>::V;
    a.n_body = body_groups<T>(a.n_vox, a.head);
    const long long threads = a.n_body + (a.n_vox - a.n_body * V);
    const long long blocks = (threads + DEC_THREADS - 1) / DEC_THREADS;
    if (blocks > INT_MAX) { *rc = FNN_E_UNSUPPORTED; return hipSuccess; }
    hipLaunchKernelGGL(decode_voxels_kernel<T>, dim3((unsigned)blocks), dim3(DEC_THREADS), 0, st, a);
    return hipGetLastError();
}

// ---- labels ------------------------------------------------------------------------------------------------------------
// The same launch shape with OB-byte labels out: a body thread's V labels are V * OB = 4 .. 32 bytes that start a multiple
// of that many bytes (at most 16) past a 16-byte boundary of `out`, stored as one dword, dwordx2 or dwordx4 (two for uint8
// voxels into 2-byte labels); `out` is only element aligned, so the body starts `head` (0 .. 16 / OB - 1) elements in.
// A voxel's flag and the largest label are reduced over the wave (ballots, shuffles) and over the block (LDS) before one
// thread of the block touches the two status words - and only when it would change them: a flag not yet set, a label above
// the maximum so far.  OR and max do not depend on the order, so both words are exact whatever is skipped.
struct LabelArgs {
    DecodeArgs d;                // (d.out unused)
    void *out;                   // OB-byte aligned; out + head * OB is 16-byte aligned
    int *status;                 // [0] flags, [1] largest valid label; zeroed on the stream before the launch
};

// the label voxel v stands for; what is none gives 0 and its one flag
template <typename T, int OB> static __device__ __forceinline__ unsigned label_of(T v, const DecodeArgs &a, int &flags, int &top) {
    constexpr int TOP = OB == 1 ? 255 : 65535;
    unsigned lab = 0;
    int flag = 0;
    bool judged = false;
    if constexpr (std::is_integral<T>::value) {
        if (!a.scale) {                                  // the integer as it is: no floating point
            if (a.byteswap) v = swap_bytes<T>(v);
            if (std::is_signed<T>::value && v < (T)0) flag = FNN_LABEL_FLAG_NEGATIVE;
            else if ((unsigned)v > (unsigned)TOP) flag = FNN_LABEL_FLAG_TOO_LARGE;
            else lab = (unsigned)v;
            judged = true;
        }
    }
    if (!judged) {
        const float f = decode_one<T>(v, a);             // the float32 fnn_decode_voxels stores
        if (!(__builtin_fabsf(f) < __builtin_inff()) || f != __builtin_truncf(f)) flag = FNN_LABEL_FLAG_NOT_INTEGRAL;
        else if (f < 0.0f) flag = FNN_LABEL_FLAG_NEGATIVE;
        else if (f > (float)TOP) flag = FNN_LABEL_FLAG_TOO_LARGE;
        else lab = (unsigned)f;                          // (-0.0 is the label 0)
    }
    flags |= flag;
    top = (int)lab > top ? (int)lab : top;
    return lab;
}

template <typename T, int OB>
__global__ __launch_bounds__(DEC_THREADS) void decode_labels_kernel(LabelArgs a) {
    constexpr int V = Group<T>::V, NO = V * OB / 4;      // dwords of labels a body thread stores
    __shared__ int block_status[2];
    if (threadIdx.x < 2) block_status[threadIdx.x] = 0;
    __syncthreads();
    const long long gid = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    int flags = 0, top = 0;
    if (gid < a.d.n_body) {
        T v[V];
        load_group<T>(a.d, gid, v);
        unsigned o[NO];
#pragma unroll
        for (int j = 0; j < NO; ++j) {
            o[j] = 0;
#pragma unroll
            for (int k = 0; k < 4 / OB; ++k) o[j] |= label_of<T, OB>(v[j * (4 / OB) + k], a.d, flags, top) << (8 * OB * k);
        }
        char *dst = (char *)a.out + (a.d.head + gid * V) * OB;
        if constexpr (NO == 1) {
            *(unsigned *)dst = o[0];
        } else if constexpr (NO == 2) {
            u32x2 q; q[0] = o[0]; q[1] = o[1];
            *(u32x2 *)dst = q;
        } else {
#pragma unroll
            for (int c = 0; c < NO / 4; ++c) {
                u32x4 q;
#pragma unroll
                for (int k = 0; k < 4; ++k) q[k] = o[4 * c + k];
                ((u32x4 *)dst)[c] = q;
            }
        }
    } else {
        // the edges: the `head` elements before the body, then everything behind it
        long long e = gid - a.d.n_body;
        if (e >= a.d.head) e += a.d.n_body * V;
        if (e < a.d.n_vox) {
            const unsigned lab = label_of<T, OB>(((const T *)a.d.raw)[e], a.d, flags, top);
            if constexpr (OB == 1) ((uint8_t *)a.out)[e] = (uint8_t)lab;
            else ((uint16_t *)a.out)[e] = (uint16_t)lab;
        }
    }
    // wave, then block, then - if it says anything new - the status words
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const int other = __shfl_xor(top, m, 64);
        top = other > top ? other : top;
    }
    flags = (__ballot(flags & 1) ? 1 : 0) | (__ballot(flags & 2) ? 2 : 0) | (__ballot(flags & 4) ? 4 : 0);
    if ((threadIdx.x & 63) == 0) {
        if (flags) atomicOr(&block_status[0], flags);
        if (top) atomicMax(&block_status[1], top);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        flags = block_status[0];
        top = block_status[1];
        if (flags & ~__atomic_load_n(&a.status[0], __ATOMIC_RELAXED)) atomicOr(&a.status[0], flags);
        if (top > __atomic_load_n(&a.status[1], __ATOMIC_RELAXED)) atomicMax(&a.status[1], top);
    }
}

template <typename T, int OB> static hipError_t launch_labels_ob(LabelArgs a, int *rc, hipStream_t st) {
    constexpr long long V = Group<T>::V;
    a.d.head = (int)(((16 - ((uintptr_t)a.out & 15)) & 15) / OB);
    if (a.d.head > a.d.n_vox) a.d.head = (int)a.d.n_vox;
    a.d.n_body = body_groups<T>(a.d.n_vox, a.d.head);
    const long long threads = a.d.n_body + (a.d.n_vox - a.d.n_body * V);
    const long long blocks = (threads + DEC_THREADS - 1) / DEC_THREADS;
    if (blocks > INT_MAX) { *rc = FNN_E_UNSUPPORTED; return hipSuccess; }
    hipLaunchKernelGGL((decode_labels_kernel<T, OB>), dim3((unsigned)blocks), dim3(DEC_THREADS), 0, st, a);
    return hipGetLastError();
}

template <typename T> static hipError_t launch_labels(const LabelArgs &a, int out_bytes, int *rc, hipStream_t st) {
    return out_bytes == 1 ? launch_labels_ob<T, 1>(a, rc, st) : launch_labels_ob<T, 2>(a, rc, st);
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
    if (int rc = fnn_need_dev("fnn_decode_voxels", {raw, out})) return rc;
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

extern "C" int fnn_decode_labels(const void *raw, int nifti_datatype, int byteswap, int64_t n_vox, int scale, double slope,
                                 double inter, int out_bytes, void *out, int32_t *status, void *stream) {
    if (!raw || !out || !status) return fnn_fail(FNN_E_INVALID, "NULL argument");
    if (n_vox < 0) return fnn_fail(FNN_E_INVALID, "negative n_vox");
    if (out_bytes != 1 && out_bytes != 2) return fnn_fail(FNN_E_INVALID, "fnn_decode_labels: out_bytes must be 1 (uint8) or 2 (uint16)");
    if ((uintptr_t)raw % 16) return fnn_fail(FNN_E_INVALID, "fnn_decode_labels: raw must be 16-byte aligned");
    if ((uintptr_t)out % out_bytes) return fnn_fail(FNN_E_INVALID, "fnn_decode_labels: out must be aligned to its element");
    if ((uintptr_t)status % 4) return fnn_fail(FNN_E_INVALID, "fnn_decode_labels: status must be 4-byte aligned");
    switch (nifti_datatype) {
    case 2: case 256: case 4: case 512: case 8: case 768: case 16: case 64: break;
    default: return fnn_fail(FNN_E_UNSUPPORTED, "fnn_decode_labels: NIfTI datatype not served (uint8, int8, int16, uint16, int32, "
                                                "uint32, float32 and float64 are)");
    }
    if (int rc = fnn_need_dev("fnn_decode_labels", {status})) return rc;
    if (n_vox > 0)
        if (int rc = fnn_need_dev("fnn_decode_labels", {raw, out})) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t r = hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st);
    if (r != hipSuccess) return fnn_fail(FNN_E_HIP, hipGetErrorString(r));
    if (n_vox == 0) return FNN_OK;
    LabelArgs a{};
    a.d.raw = raw; a.d.n_vox = n_vox;
    a.d.byteswap = byteswap != 0; a.d.scale = scale != 0;
    a.d.slope = slope; a.d.inter = inter;
    a.d.mul = slope != 1.0; a.d.add = inter != 0.0;
    a.out = out; a.status = status;
    int rc = FNN_OK;
    switch (nifti_datatype) {
    case 2: r = launch_labels<uint8_t>(a, out_bytes, &rc, st); break;
    case 256: r = launch_labels<int8_t>(a, out_bytes, &rc, st); break;
    case 4: r = launch_labels<int16_t>(a, out_bytes, &rc, st); break;
    case 512: r = launch_labels<uint16_t>(a, out_bytes, &rc, st); break;
    case 8: r = launch_labels<int32_t>(a, out_bytes, &rc, st); break;
    case 768: r = launch_labels<uint32_t>(a, out_bytes, &rc, st); break;
    case 16: r = launch_labels<float>(a, out_bytes, &rc, st); break;
    default: r = launch_labels<double>(a, out_bytes, &rc, st); break;
    }
    if (rc != FNN_OK) return fnn_fail(rc, "fnn_decode_labels: too many voxels for one launch");
    if (r != hipSuccess) return fnn_fail(FNN_E_HIP, hipGetErrorString(r));
    return FNN_OK;
}
