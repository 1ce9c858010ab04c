// resample_torch.hip - the torch resampling family of nnU-Net (resample_torch_fornnunet,
// preprocessing/resampling/resample_torch.py:96-154), gfx950.
//
// The reference calls torch.nn.functional.interpolate(x[None].float(), size, mode='trilinear', antialias=False), i.e.
// align_corners=False, per axis (all float32)
//     scale = (float)in / (float)out,   src = max(fmaf(scale, o + 0.5f, -0.5f), 0),
//     i0 = min((int)src, in - 1),       i1 = i0 + (i0 < in - 1),     l1 = src - i0,   l0 = 1 - l1,
// an axis with in == out being the identity; along an anisotropic axis (separate_axis) it takes the 'nearest-exact' slice
//     idx = min((int)floorf((o + 0.5f) * scale), in - 1)
// after blending in the plane.  Picking the slice first and blending in the plane is the same arithmetic, so both of the
// reference's passes are one pass here: one thread per output voxel (z fastest), taps and weights computed once, the
// channels looped inside the thread.  No staging buffer, no fp64, no allocation; the coordinate is one explicit
// __fmaf_rn so that the compiler's contraction setting cannot change it.
//
// Rows of 64 or more output voxels over at most 512 input voxels (the logit export) take rt_rows_kernel instead: one
// wave per output row, the four input rows it blends staged in LDS by coalesced loads (the next channel's on their way
// while this one is blended), so an input voxel is fetched once per output row instead of once per tap.  Same
// arithmetic in the same order: the two kernels give the same bits.
//
// Segmentations (resample_torch_simple, :51-85): per unique label u, ascending, the reference interpolates
// (seg == u) * 1000 into fp16 scores; voxels above 700 take u, the rest the argmax over the scores, first maximum winning -
// which is the argmax of the fp16-rounded scores with the smallest label winning ties (a score above 700 leaves less than
// 300 for everyone else).  Only the labels at the 8 taps (4 in the plane) can score above 0, so a thread gathers those,
// evaluates the score of every distinct one in registers and picks: no one-hot tensor, no unique(), no buffer.
// memefficient_seg_resampling=True is the other rule: the float32 score of (seg == u) above 0.5 takes the label, else 0.
#include "resample_torch_common.h"
#include "host_call.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void rt_image_kernel(const T *__restrict__ in, RGeo g, int C, T *__restrict__ out) {
    const Taps t = make_taps(g);
    if (!t.live) return;
    const long long nin = g.in[0] * g.in[1] * g.in[2], nout = g.out[0] * (long long)g.plane;
#pragma unroll 2
    for (int c = 0; c < C; ++c) {
        const T *p = in + (long long)c * nin;
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (float)p[t.off[k]];
        out[(long long)c * nout + t.o] = store_cast<T>(blend(t, v));
    }
}

constexpr int ROWS_MAX_IN = 512, ROWS_PER_LANE = ROWS_MAX_IN / 64, ROWS_MIN_OUT = 64;

template <typename T>
__global__ __launch_bounds__(256) void rt_rows_kernel(const T *__restrict__ in, RGeo g, int C, T *__restrict__ out) {
    extern __shared__ unsigned char rows_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int inz = (int)g.in[2], outz = (int)g.out[2];
    T *rows = reinterpret_cast<T *>(rows_lds) + (size_t)wave * 4 * inz;          // this wave's [4][inz]
    const unsigned n_rows = (unsigned)(g.out[0] * g.out[1]);
    unsigned row = blockIdx.x * 4u + wave;
    const bool live = row < n_rows;
    row = live ? row : n_rows - 1;                                                // the barriers stay uniform; no store
    const unsigned ox = row / (unsigned)g.out[1], oy = row - ox * (unsigned)g.out[1];
    Taps t;
    long long x[2], y[2], z[2];
    axis_taps(g, 0, ox, x[0], x[1], t.wx0, t.wx1);
    axis_taps(g, 1, oy, y[0], y[1], t.wy0, t.wy1);
    long long base[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) base[r] = (x[r >> 1] * g.in[1] + y[r & 1]) * inz;
    const long long nin = g.in[0] * g.in[1] * g.in[2], nout = g.out[0] * (long long)g.plane;
    T *orow = out + (long long)row * outz;
    T reg[4][ROWS_PER_LANE];
    auto fetch = [&](int c) {
        const T *p = in + (long long)c * nin;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < ROWS_PER_LANE; ++j) {
                const int zi = lane + 64 * j;
                if (zi < inz) reg[r][j] = p[base[r] + zi];
            }
    };
    fetch(0);
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < ROWS_PER_LANE; ++j) {
                const int zi = lane + 64 * j;
                if (zi < inz) rows[r * inz + zi] = reg[r][j];
            }
        __syncthreads();
        if (c + 1 < C) fetch(c + 1);
        for (int oz = lane; oz < outz; oz += 64) {
            axis_taps(g, 2, oz, z[0], z[1], t.wz0, t.wz1);
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (float)rows[(k >> 1) * inz + (int)z[k & 1]];
            if (live) orow[(long long)c * nout + oz] = store_cast<T>(blend(t, v));
        }
        __syncthreads();
    }
}

template <typename T>
static void launch_image(const T *in, const RGeo &g, int C, T *out, hipStream_t st) {
    const long long n_rows = g.out[0] * g.out[1];
    if (g.in[2] <= ROWS_MAX_IN && g.out[2] >= ROWS_MIN_OUT && n_rows < (1LL << 31)) {
        const size_t lds = (size_t)4 * 4 * g.in[2] * sizeof(T);                  // <= 32 KiB
        hipLaunchKernelGGL(rt_rows_kernel<T>, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), lds, st, in, g, C, out);
    } else {
        hipLaunchKernelGGL(rt_image_kernel<T>, dim3(g.plane_blocks * (unsigned)g.out[0]), dim3(256), 0, st, in, g, C, out);
    }
}

template <bool MEMEFF>
__global__ __launch_bounds__(256) void rt_seg_kernel(const short *__restrict__ in, RGeo g, int C, short *__restrict__ out) {
    const Taps t = make_taps(g);
    if (!t.live) return;
    const long long nin = g.in[0] * g.in[1] * g.in[2], nout = g.out[0] * (long long)g.plane;
    const float one = MEMEFF ? 1.f : 1000.f;
    for (int c = 0; c < C; ++c) {
        const short *p = in + (long long)c * nin;
        short l[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) l[k] = p[t.off[k]];
        short best = 0;
        float best_s = -1.f;
        bool any = false;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            bool seen = false;
#pragma unroll
            for (int j = 0; j < k; ++j) seen |= l[j] == l[k];
            if (seen) continue;
            float e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = l[j] == l[k] ? one : 0.f;
            float s = blend(t, e);
            if (MEMEFF) {
                if (s > 0.5f && (!any || l[k] > best)) { best = l[k]; any = true; }      // labels ascending: the last one stays
            } else {
                s = (float)store_cast<f16>(s);                                                     // the fp16 score tensor
                if (s > best_s || (s == best_s && l[k] < best)) { best = l[k]; best_s = s; }
            }
        }
        out[(long long)c * nout + t.o] = best;
    }
}

static int check_args(const void *in, const int64_t *shape, const int64_t *new_shape, const fnn_resample_torch_desc *d,
                      const void *out) {
    if (!in || !shape || !new_shape || !d || !out) return fnn_fail(FNN_E_INVALID, "NULL argument");
    if (d->mode != FNN_INTERP_LINEAR) return fnn_fail(FNN_E_UNSUPPORTED, "mode other than 'linear' is not implemented");
    if (d->aniso_axis_mode != FNN_INTERP_NEAREST_EXACT) return fnn_fail(FNN_E_UNSUPPORTED, "aniso_axis_mode other than 'nearest-exact' is not implemented");
    if (d->separate_axis < -1 || d->separate_axis > 2) return fnn_fail(FNN_E_INVALID, "separate_axis must be -1 .. 2");
    for (int a = 0; a < 4; ++a) if (shape[a] < 1) return fnn_fail(FNN_E_INVALID, "bad shape");
    for (int a = 0; a < 3; ++a) if (new_shape[a] < 1) return fnn_fail(FNN_E_INVALID, "bad new_shape");
    if (!fnn_dev_ptr(in) || !fnn_dev_ptr(out)) return fnn_fail(FNN_E_INVALID, "the torch resampling kernels need device pointers (no CPU path)");
    return FNN_OK;
}

}  // namespace

extern "C" int fnn_resample_torch(const void *in, const int64_t shape[4], const int64_t new_shape[3],
                                  const fnn_resample_torch_desc *d, void *out, void *stream) {
    int rc = check_args(in, shape, new_shape, d, out);
    if (rc != FNN_OK) return rc;
    if ((rc = fnn_check_float_dtype(d->dtype)) != FNN_OK) return rc;
    RGeo g{};
    const char *why = "";
    if ((rc = rt_geometry(shape, new_shape, d->separate_axis, g, &why)) != FNN_OK) return fnn_fail(rc, why);
    hipStream_t st = (hipStream_t)stream;
    fnn_by_float(d->dtype, [&](auto t) { using T = decltype(t); launch_image((const T *)in, g, (int)shape[0], (T *)out, st); });
    if (hipGetLastError() != hipSuccess) return fnn_fail(FNN_E_HIP, "fnn_resample_torch: launch failed");
    return FNN_OK;
}

extern "C" int fnn_resample_torch_seg(const int16_t *in, const int64_t shape[4], const int64_t new_shape[3],
                                      const fnn_resample_torch_desc *d, int16_t *out, void *stream) {
    int rc = check_args(in, shape, new_shape, d, out);
    if (rc != FNN_OK) return rc;
    RGeo g{};
    const char *why = "";
    if ((rc = rt_geometry(shape, new_shape, d->separate_axis, g, &why)) != FNN_OK) return fnn_fail(rc, why);
    const dim3 grid(g.plane_blocks * (unsigned)g.out[0]), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (d->memefficient) hipLaunchKernelGGL(rt_seg_kernel<true>, grid, block, 0, st, (const short *)in, g, (int)shape[0], (short *)out);
    else hipLaunchKernelGGL(rt_seg_kernel<false>, grid, block, 0, st, (const short *)in, g, (int)shape[0], (short *)out);
    if (hipGetLastError() != hipSuccess) return fnn_fail(FNN_E_HIP, "fnn_resample_torch_seg: launch failed");
    return FNN_OK;
}
