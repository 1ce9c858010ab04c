// export_labels.hip - labels on the cropped grid straight from the logits of the network grid (fnn_resample_labels), gfx950.
//
// The export of a case whose file spacing differs from the plan's (export_prediction.py:26-53) resamples the logits
// [heads][network grid] to shape_after_cropping_and_before_resampling and takes the label rule over the result.  Done in
// two steps the resampled tensor is written and read back once: heads * n_out values that nobody else wants.  Here one
// thread owns an output voxel, computes its taps and weights once, and walks the heads: each head's value is interpolated
// in registers, rounded to the logits' dtype as the resampler would have stored it, and fed to LabelPick
// (output_common.h).  One launch, no scratch memory, no allocation, no synchronisation.
//
// The labels are bit for bit those of fnn_resample (order 1, order_z 0) / fnn_resample_torch followed by
// fnn_argmax_labels, so each family's value is formed by the expressions of its resampler in their order:
//
// default family (interp_kernel of resample.hip at order 1, fp64): per axis x = fma(o, zoom, 0.5 * zoom - 0.5) clamped to
//   [0, in - 1], taps floor(x) and floor(x) + 1 (index clamped) with weights 1 - t and t; an axis with in == out is one
//   tap of weight 1; the separate axis is the order-0 pick floor(fma(o + 0.5, zoom, -0.5) + 0.5), clamped.  The sum starts
//   at 0 and adds the taps in C order as fma((c * w0) * w1, w2, sum).  A factor of exactly 1 is left out (c * 1 = c and
//   fma(t, 1, s) = s + t for every c, NaN and infinities included) - but a single-tap axis never becomes a second tap of
//   weight 0 (inf * 0 is NaN and interp_kernel does not form it there), while the weight-0 upper tap of an interpolating
//   axis at its high edge, which interp_kernel does form, is kept.
//   fnn_resample's clip to the channel's (slice's) input range is not applied: at order 1 the sum is a convex blend in
//   fp64 of values of the logits' dtype, it leaves their range by ~1e-16 relative at most, and the rounding to that dtype
//   returns the bound itself (pinned by the plateau cases of tests/test_gpu_export_labels.py).
// torch family (rt_image_kernel of resample_torch.hip, float32): resample_torch_common.h as it is - there an axis with
//   in == out is blended with its own value at weight 0 (that is what the resampler computes), only the second load of
//   the same address is dropped.
//
// The kernels are specialised on which axes have two taps (mask M: bit a = axis a), so that taps and weights stay in
// registers under compile-time indices.
#include "output_common.h"
#include "resample_default_common.h"
#include "resample_torch_common.h"
#include "host_call.h"
#include <type_traits>

namespace {

constexpr int HEADS_IN_FLIGHT = 4;     // heads whose tap loads are issued before the first of them is blended

template <typename T> struct Name;
template <> struct Name<f16> { static constexpr const char *v = "f16"; };
template <> struct Name<float> { static constexpr const char *v = "f32"; };

// ---- default family ---------------------------------------------------------------------------------------------------
// DGeo, d_axis and d_value: resample_default_common.h
template <typename T, int M>
__global__ __launch_bounds__(256) void export_labels_default_kernel(const T *__restrict__ in, DGeo g, int heads,
                                                                    const int *__restrict__ order, void *labels, int label_u16) {
    const unsigned ox = blockIdx.x / g.plane_blocks;
    const unsigned j = (blockIdx.x - ox * g.plane_blocks) * 256u + threadIdx.x;
    if (j >= g.plane) return;
    const unsigned oy = j / (unsigned)g.out[2], oz = j - oy * (unsigned)g.out[2];
    long long i[3][2];
    double w[3][2];
    d_axis<(M & 1) != 0>(g, 0, ox, i[0], w[0]);
    d_axis<(M & 2) != 0>(g, 1, oy, i[1], w[1]);
    d_axis<(M & 4) != 0>(g, 2, oz, i[2], w[2]);
    long long off[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) off[k] = (i[0][k >> 2] * g.in[1] + i[1][(k >> 1) & 1]) * g.in[2] + i[2][k & 1];
    constexpr int KM = ((M & 1) ? 4 : 0) | (M & 2) | ((M & 4) ? 1 : 0);      // the tap indices that are loaded
    const long long nin = g.in[0] * g.in[1] * g.in[2];
    const T *p = in;
    LabelPick pick;
    int h = 0;
    for (; h + HEADS_IN_FLIGHT <= heads; h += HEADS_IN_FLIGHT) {
        T v[HEADS_IN_FLIGHT][8];
#pragma unroll
        for (int u = 0; u < HEADS_IN_FLIGHT; ++u) {
#pragma unroll
            for (int k = 0; k < 8; ++k) if ((k & ~KM) == 0) v[u][k] = p[off[k]];
            p += nin;
        }
#pragma unroll
        for (int u = 0; u < HEADS_IN_FLIGHT; ++u) pick.feed(h + u, d_value<T, M>(v[u], w));
    }
    for (; h < heads; ++h) {
        T v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) if ((k & ~KM) == 0) v[k] = p[off[k]];
        p += nin;
        pick.feed(h, d_value<T, M>(v, w));
    }
    store_label(labels, label_u16, (size_t)ox * g.plane + j, pick.label(order));
}

// ---- torch family -----------------------------------------------------------------------------------------------------
template <typename T, int M>
__global__ __launch_bounds__(256) void export_labels_torch_kernel(const T *__restrict__ in, RGeo g, int heads,
                                                                  const int *__restrict__ order, void *labels, int label_u16) {
    const Taps t = make_taps(g);
    if (!t.live) return;
    constexpr int KM = ((M & 1) ? 4 : 0) | (M & 2) | ((M & 4) ? 1 : 0);      // a corner outside it repeats corner k & KM
    const long long nin = g.in[0] * g.in[1] * g.in[2];
    const T *p = in;
    LabelPick pick;
    int h = 0;
    for (; h + HEADS_IN_FLIGHT <= heads; h += HEADS_IN_FLIGHT) {
        T r[HEADS_IN_FLIGHT][8];
#pragma unroll
        for (int u = 0; u < HEADS_IN_FLIGHT; ++u) {
#pragma unroll
            for (int k = 0; k < 8; ++k) if ((k & ~KM) == 0) r[u][k] = p[t.off[k]];
            p += nin;
        }
#pragma unroll
        for (int u = 0; u < HEADS_IN_FLIGHT; ++u) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (float)r[u][k & KM];
            pick.feed(h + u, (float)store_cast<T>(blend(t, v)));
        }
    }
    for (; h < heads; ++h) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) if ((k & ~KM) == 0) v[k] = (float)p[t.off[k]];
#pragma unroll
        for (int k = 0; k < 8; ++k) if ((k & ~KM) != 0) v[k] = v[k & KM];
        p += nin;
        pick.feed(h, (float)store_cast<T>(blend(t, v)));
    }
    store_label(labels, label_u16, (size_t)t.o, pick.label(order));
}

template <typename T, int M, typename G>
static void launch_one(const T *in, const G &g, int heads, const int *order, void *labels, int label_u16, hipStream_t st) {
    const dim3 grid(g.plane_blocks * (unsigned)g.out[0]), block(256);
    if constexpr (std::is_same<G, DGeo>::value) {
        fnn_note_kernel("export_labels_default_kernel<%s,%d>", Name<T>::v, M);
        hipLaunchKernelGGL((export_labels_default_kernel<T, M>), grid, block, 0, st, in, g, heads, order, labels, label_u16);
    } else {
        fnn_note_kernel("export_labels_torch_kernel<%s,%d>", Name<T>::v, M);
        hipLaunchKernelGGL((export_labels_torch_kernel<T, M>), grid, block, 0, st, in, g, heads, order, labels, label_u16);
    }
}

template <typename T, typename G>
static void launch(int mask, const T *in, const G &g, int heads, const int *order, void *labels, int label_u16, hipStream_t st) {
    switch (mask) {
        case 0: launch_one<T, 0>(in, g, heads, order, labels, label_u16, st); break;
        case 1: launch_one<T, 1>(in, g, heads, order, labels, label_u16, st); break;
        case 2: launch_one<T, 2>(in, g, heads, order, labels, label_u16, st); break;
        case 3: launch_one<T, 3>(in, g, heads, order, labels, label_u16, st); break;
        case 4: launch_one<T, 4>(in, g, heads, order, labels, label_u16, st); break;
        case 5: launch_one<T, 5>(in, g, heads, order, labels, label_u16, st); break;
        case 6: launch_one<T, 6>(in, g, heads, order, labels, label_u16, st); break;
        default: launch_one<T, 7>(in, g, heads, order, labels, label_u16, st); break;
    }
}

}  // namespace

extern "C" int fnn_resample_labels(const void *logits, int dtype, const int64_t shape[4], const int64_t new_shape[3],
                                   int family, int separate_axis, const int32_t *regions_class_order, int n_regions,
                                   void *labels, int label_dtype, void *stream) {
    if (!logits || !shape || !new_shape || !labels) return fnn_fail(FNN_E_INVALID, "NULL argument");
    if (family != FNN_RESAMPLE_DEFAULT && family != FNN_RESAMPLE_TORCH) return fnn_fail(FNN_E_UNSUPPORTED, "unknown resampling family");
    if (int rc = fnn_check_float_dtype(dtype)) return rc;
    if (int rc = fnn_check_label_dtype(label_dtype)) return rc;
    if (separate_axis < -1 || separate_axis > 2) return fnn_fail(FNN_E_INVALID, "separate_axis must be -1 .. 2");
    if (shape[0] < 1) return fnn_fail(FNN_E_INVALID, "heads must be at least 1");
    for (int a = 1; a < 4; ++a) if (shape[a] < 1) return fnn_fail(FNN_E_INVALID, "bad shape");
    for (int a = 0; a < 3; ++a) if (new_shape[a] < 1) return fnn_fail(FNN_E_INVALID, "bad new_shape");
    if (regions_class_order && n_regions != shape[0]) return fnn_fail(FNN_E_INVALID, "regions_class_order needs one entry per head");
    if (!regions_class_order && label_dtype == FNN_LABEL_U8 && shape[0] > 256) return fnn_fail(FNN_E_INVALID, "more than 256 heads need uint16 labels");
    if (int rc = fnn_need_dev("fnn_resample_labels", {logits, labels})) return rc;
    if (regions_class_order)
        if (int rc = fnn_need_dev("fnn_resample_labels", {regions_class_order})) return rc;
    RGeo rg{};                                                 // the grid rule and its limits are the torch family's for both
    const char *why = "";
    if (int rc = rt_geometry(shape, new_shape, separate_axis, rg, &why)) return fnn_fail(rc, why);
    int mask = 0;
    for (int a = 0; a < 3; ++a) if (shape[1 + a] != new_shape[a] && a != separate_axis) mask |= 1 << a;
    const int heads = (int)shape[0], u16 = label_dtype == FNN_LABEL_U16;
    const int *order = (const int *)regions_class_order;
    hipStream_t st = (hipStream_t)stream;
    fnn_op_klog_begin();                                       // the kernel's name for fnn_op_last_kernels
    if (family == FNN_RESAMPLE_TORCH) {
        if (dtype == FNN_OUT_F32) launch(mask, (const float *)logits, rg, heads, order, labels, u16, st);
        else launch(mask, (const f16 *)logits, rg, heads, order, labels, u16, st);
    } else {
        DGeo g{};
        g.sep = separate_axis; g.plane = rg.plane; g.plane_blocks = rg.plane_blocks;
        for (int a = 0; a < 3; ++a) { g.in[a] = rg.in[a]; g.out[a] = rg.out[a]; g.zoom[a] = (double)g.in[a] / (double)g.out[a]; }
        if (dtype == FNN_OUT_F32) launch(mask, (const float *)logits, g, heads, order, labels, u16, st);
        else launch(mask, (const f16 *)logits, g, heads, order, labels, u16, st);
    }
    fnn_op_klog_end();
    if (hipGetLastError() != hipSuccess) return fnn_fail(FNN_E_HIP, "fnn_resample_labels: launch failed");
    return FNN_OK;
}
