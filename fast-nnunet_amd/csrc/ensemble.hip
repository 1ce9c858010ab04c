// ensemble.hip - nnU-Net's cross-configuration ensembling on the device, gfx950.
//
//   fnn_ensemble_export         every member's logits of the cropped grid -> the member's probabilities exactly as
//                               export_prob_kernel (prep.hip) computes them -> average_probabilities
//                               (ensembling/ensemble.py:16-28) -> LabelManager.convert_logits_to_segmentation of the
//                               average (ensemble.py:42, label_handling.py:183-195), on the raw grid, in one pass
//   fnn_average_probabilities   the same average and label rule on probabilities the caller already holds
//
// The average is p_0, then += p_m in member order, then / (float)N: numpy's `avg = p0.astype(f32); avg += p_i; avg /= n`
// element for element, so the result is bit-identical to it.  Nothing may be contracted into an FMA: the pragma below
// keeps every product, sum and quotient a separate IEEE operation whatever -ffp-contract the build passes.
//
// Both kernels are HBM-bound.  A thread owns VEC consecutive voxels; with the identity transpose and rows that are
// multiples of 4 (the common case) VEC = 4: 8-byte (fp16) or 16-byte (fp32) loads per member and head, 16-byte stores
// of the average.  The softmax needs three passes over a member's heads (max, sum, probability); the first reads the
// logits from HBM, the other two re-read the same lines, as export_prob_kernel does.
#include "ensemble_common.h"
#include "host_call.h"
#include <climits>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int ENS_THREADS = 256;
constexpr int ENS_VEC_MAX_MEMBERS = 8;           // the VEC = 4 kernels keep 2 x 4 floats of softmax state per member

struct EnsembleArgs {
    const void *member[ENS_MAX_MEMBERS];     // [H][e0][e1][e2] logits (export) / [H][n] float32 probabilities (average)
    unsigned f32_mask;                       // bit m: member m is float32 (else fp16)
    int N, H;
    const int *order;                        // regions_class_order on the device, or nullptr for plain labels
    CropBox box;                             // export: crop box (transposed axes) and output grid
    float *avg;                              // [H][o0][o1][o2] or nullptr
};

// VEC consecutive elements of member m from element idx (idx and the member's base aligned to VEC elements)
template <int VEC>
static __device__ __forceinline__ void load_member(const EnsembleArgs &a, int m, size_t idx, float x[VEC]) {
    if (a.f32_mask >> m & 1u) {
        const float *p = (const float *)a.member[m] + idx;
        if constexpr (VEC == 4) {
            const f32x4 v = *(const f32x4 *)p;
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = v[k];
        } else {
            x[0] = p[0];
        }
    } else {
        const f16 *p = (const f16 *)a.member[m] + idx;
        if constexpr (VEC == 4) {
            const f16x4 v = *(const f16x4 *)p;
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = (float)v[k];
        } else {
            x[0] = (float)p[0];
        }
    }
}

template <int VEC>
static __device__ __forceinline__ void store_avg(float *avg, size_t idx, const float v[VEC]) {
    if constexpr (VEC == 4) {
        *(f32x4 *)(avg + idx) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
        avg[idx] = v[0];
    }
}

template <int VEC, typename LT>
static __device__ __forceinline__ void store_labels(LT *labels, size_t idx, const int v[VEC]) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) labels[idx + k] = (LT)v[k];
}

// the merge rule on the averaged value of head h: ensemble_common.h
static __device__ __forceinline__ void merge_rule(const EnsembleArgs &a, int h, float v, float &best, int &label) {
    ensemble_merge_rule(a.order, h, v, best, label);
}

// ---- N members' logits [H][e0][e1][e2] (transposed, cropped grid) -> average probabilities [H][o0][o1][o2] (optional)
// + labels [o0][o1][o2] on the raw grid.  Member m's probability of head h is export_prob_kernel's expression for it.
template <int VEC, int MAXN, typename LT>
__global__ __launch_bounds__(ENS_THREADS) void ensemble_export_kernel(EnsembleArgs a, LT *labels) {
    const long long n = a.box.o[0] * a.box.o[1] * a.box.o[2];
    const long long i = ((long long)blockIdx.x * ENS_THREADS + threadIdx.x) * VEC;
    if (i >= n) return;
    size_t v;
    const bool inside = crop_box_voxel(a.box, i, v);
    int label[VEC];
    float best[VEC], acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { label[k] = 0; best[k] = -1.f; }
    // VEC = 4 only runs when the box's z edges and the rows are multiples of 4: the 4 voxels are all in or all out
    if (!inside) {
        // every member's probability is 1 for the background / 0 elsewhere (revert_cropping_on_probabilities, 0 for
        // every region), so the average is too, and both rules give label 0
        if (a.avg)
            for (int h = 0; h < a.H; ++h) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = (!a.order && h == 0) ? 1.f : 0.f;
                store_avg<VEC>(a.avg, (size_t)h * n + i, acc);
            }
        store_labels<VEC, LT>(labels, i, label);
        return;
    }
    const size_t plane = (size_t)a.box.e[0] * a.box.e[1] * a.box.e[2];
    const float fn = (float)a.N;
    float x[VEC];
    if (a.order) {
        for (int h = 0; h < a.H; ++h) {
#pragma unroll
            for (int m = 0; m < MAXN; ++m) {
                if (m >= a.N) break;
                load_member<VEC>(a, m, h * plane + v, x);
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float p = 1.f / (1.f + expf(-x[k]));
                    acc[k] = m == 0 ? p : acc[k] + p;
                }
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = acc[k] / fn;
            if (a.avg) store_avg<VEC>(a.avg, (size_t)h * n + i, acc);
#pragma unroll
            for (int k = 0; k < VEC; ++k) merge_rule(a, h, acc[k], best[k], label[k]);
        }
        store_labels<VEC, LT>(labels, i, label);
        return;
    }
    // softmax state of every member: max over the heads in head order, then sum += expf(x - max) from 0.f
    float mx[MAXN][VEC], sum[MAXN][VEC];
#pragma unroll
    for (int m = 0; m < MAXN; ++m) {
        if (m >= a.N) break;
        load_member<VEC>(a, m, v, x);
#pragma unroll
        for (int k = 0; k < VEC; ++k) { mx[m][k] = x[k]; sum[m][k] = 0.f; }
        for (int h = 1; h < a.H; ++h) {
            load_member<VEC>(a, m, h * plane + v, x);
#pragma unroll
            for (int k = 0; k < VEC; ++k) mx[m][k] = fmaxf(mx[m][k], x[k]);
        }
        for (int h = 0; h < a.H; ++h) {
            load_member<VEC>(a, m, h * plane + v, x);
#pragma unroll
            for (int k = 0; k < VEC; ++k) sum[m][k] += expf(x[k] - mx[m][k]);
        }
    }
    for (int h = 0; h < a.H; ++h) {
#pragma unroll
        for (int m = 0; m < MAXN; ++m) {
            if (m >= a.N) break;
            load_member<VEC>(a, m, h * plane + v, x);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float p = expf(x[k] - mx[m][k]) / sum[m][k];
                acc[k] = m == 0 ? p : acc[k] + p;
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = acc[k] / fn;
        if (a.avg) store_avg<VEC>(a.avg, (size_t)h * n + i, acc);
#pragma unroll
        for (int k = 0; k < VEC; ++k) merge_rule(a, h, acc[k], best[k], label[k]);
    }
    store_labels<VEC, LT>(labels, i, label);
}

// ---- N float32 probability buffers [H][n] -> average [H][n] (optional) + labels [n]
template <int VEC, typename LT>
__global__ __launch_bounds__(ENS_THREADS) void average_probabilities_kernel(EnsembleArgs a, long long n, LT *labels) {
    const long long i = ((long long)blockIdx.x * ENS_THREADS + threadIdx.x) * VEC;
    if (i >= n) return;
    int label[VEC];
    float best[VEC], acc[VEC], x[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { label[k] = 0; best[k] = -1.f; }
    const float fn = (float)a.N;
    for (int h = 0; h < a.H; ++h) {
        for (int m = 0; m < a.N; ++m) {
            load_member<VEC>(a, m, (size_t)h * n + i, x);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = m == 0 ? x[k] : acc[k] + x[k];
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = acc[k] / fn;
        if (a.avg) store_avg<VEC>(a.avg, (size_t)h * n + i, acc);
#pragma unroll
        for (int k = 0; k < VEC; ++k) merge_rule(a, h, acc[k], best[k], label[k]);
    }
    store_labels<VEC, LT>(labels, i, label);
}

static bool aligned(const void *p, size_t bytes) { return ((uintptr_t)p % bytes) == 0; }

}  // namespace

extern "C" {

int fnn_ensemble_export(const void *const *member_logits, const int32_t *member_dtype, int n_members, int heads,
                        const int32_t *regions_class_order, const int64_t bbox[6], const int64_t shape_before_cropping[3],
                        const int32_t transpose_backward[3], float *avg_probs, void *labels, int label_dtype, void *stream) {
    if (!member_logits || !member_dtype || !bbox || !shape_before_cropping || !transpose_backward || !labels)
        return fnn_fail(FNN_E_INVALID, "NULL argument");
    if (n_members < 1 || n_members > ENS_MAX_MEMBERS) return fnn_fail(FNN_E_INVALID, "n_members must be 1..16");
    for (int m = 0; m < n_members; ++m) {
        if (!member_logits[m]) return fnn_fail(FNN_E_INVALID, "NULL member logits");
        if (int rc = fnn_check_float_dtype(member_dtype[m], "member logits dtype")) return rc;
    }
    if (heads < 1 || heads > 4096) return fnn_fail(FNN_E_INVALID, "bad number of heads");
    if (int rc = fnn_check_label_dtype(label_dtype)) return rc;
    if (int rc = fnn_check_perm(transpose_backward, "transpose_backward")) return rc;
    EnsembleArgs a{};
    if (int rc = crop_box_fill(a.box, bbox, shape_before_cropping, transpose_backward)) return rc;
    for (int m = 0; m < n_members; ++m)
        if (int rc = fnn_need_dev("fnn_ensemble_export", {member_logits[m]})) return rc;
    if (int rc = fnn_need_dev("fnn_ensemble_export", {labels})) return rc;
    if (avg_probs)
        if (int rc = fnn_need_dev("fnn_ensemble_export", {avg_probs})) return rc;
    a.N = n_members; a.H = heads; a.avg = avg_probs;
    for (int m = 0; m < n_members; ++m) {
        a.member[m] = member_logits[m];
        if (member_dtype[m] == FNN_OUT_F32) a.f32_mask |= 1u << m;
    }
    const CropBox &b = a.box;
    const size_t lbytes = label_dtype == FNN_LABEL_U16 ? 2 : 1;
    bool vec = b.tb[0] == 0 && b.tb[1] == 1 && b.tb[2] == 2 && b.o[2] % 4 == 0 && b.lo[2] % 4 == 0 && b.e[2] % 4 == 0 &&
               n_members <= ENS_VEC_MAX_MEMBERS && aligned(labels, 4 * lbytes) && (!avg_probs || aligned(avg_probs, 16));
    for (int m = 0; m < n_members; ++m) vec = vec && aligned(member_logits[m], 16);
    const long long n = b.o[0] * b.o[1] * b.o[2];
    const int V = vec ? 4 : 1;
    if ((n / V + ENS_THREADS - 1) / ENS_THREADS > UINT_MAX) return fnn_fail(FNN_E_UNSUPPORTED, "output grid too large");
    HipCall call(stream);
    const DevBuf order = upload_order(regions_class_order, heads, call);
    a.order = order.as<int>();
    const dim3 grid((unsigned)((n / V + ENS_THREADS - 1) / ENS_THREADS));
    fnn_by_label(label_dtype, [&](auto lt) {
        using LT = decltype(lt);
        if (vec) call.launch(ensemble_export_kernel<4, ENS_VEC_MAX_MEMBERS, LT>, grid, dim3(ENS_THREADS), 0, a, (LT *)labels);
        else call.launch(ensemble_export_kernel<1, ENS_MAX_MEMBERS, LT>, grid, dim3(ENS_THREADS), 0, a, (LT *)labels);
    });
    return call.finish();
}

int fnn_average_probabilities(const float *const *member_probs, int n_members, int heads, const int32_t *regions_class_order,
                              int64_t n_vox, float *avg_probs, void *labels, int label_dtype, void *stream) {
    if (!member_probs || !labels) return fnn_fail(FNN_E_INVALID, "NULL argument");
    if (n_members < 1 || n_members > ENS_MAX_MEMBERS) return fnn_fail(FNN_E_INVALID, "n_members must be 1..16");
    for (int m = 0; m < n_members; ++m)
        if (!member_probs[m]) return fnn_fail(FNN_E_INVALID, "NULL member probabilities");
    if (heads < 1 || heads > 4096) return fnn_fail(FNN_E_INVALID, "bad number of heads");
    if (int rc = fnn_check_label_dtype(label_dtype)) return rc;
    if (n_vox < 0) return fnn_fail(FNN_E_INVALID, "negative n_vox");
    if (n_vox == 0) return FNN_OK;
    for (int m = 0; m < n_members; ++m)
        if (int rc = fnn_need_dev("fnn_average_probabilities", {member_probs[m]})) return rc;
    if (int rc = fnn_need_dev("fnn_average_probabilities", {labels})) return rc;
    if (avg_probs)
        if (int rc = fnn_need_dev("fnn_average_probabilities", {avg_probs})) return rc;
    EnsembleArgs a{};
    a.N = n_members; a.H = heads; a.avg = avg_probs;
    const size_t lbytes = label_dtype == FNN_LABEL_U16 ? 2 : 1;
    bool vec = n_vox % 4 == 0 && aligned(labels, 4 * lbytes) && (!avg_probs || aligned(avg_probs, 16));
    for (int m = 0; m < n_members; ++m) {
        a.member[m] = member_probs[m];
        a.f32_mask |= 1u << m;
        vec = vec && aligned(member_probs[m], 16);
    }
    const int V = vec ? 4 : 1;
    if ((n_vox / V + ENS_THREADS - 1) / ENS_THREADS > UINT_MAX) return fnn_fail(FNN_E_UNSUPPORTED, "too many voxels");
    HipCall call(stream);
    const DevBuf order = upload_order(regions_class_order, heads, call);
    a.order = order.as<int>();
    const dim3 grid((unsigned)((n_vox / V + ENS_THREADS - 1) / ENS_THREADS));
    fnn_by_label(label_dtype, [&](auto lt) {
        using LT = decltype(lt);
        if (vec) call.launch(average_probabilities_kernel<4, LT>, grid, dim3(ENS_THREADS), 0, a, (long long)n_vox, (LT *)labels);
        else call.launch(average_probabilities_kernel<1, LT>, grid, dim3(ENS_THREADS), 0, a, (long long)n_vox, (LT *)labels);
    });
    return call.finish();
}

}  // extern "C"
