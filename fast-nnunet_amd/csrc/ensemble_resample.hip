// ensemble_resample.hip - fnn_ensemble_export straight from the members' network grids (fnn_ensemble_resample_export), gfx950.
//
// Members of an ensemble of configurations live on different grids (3d_fullres + 3d_lowres, 2d + 3d_fullres), so on the
// way to fnn_ensemble_export at least one member's logits are resampled to the cropped grid and written: heads * cropped
// voxels values per member that are written once and read three times.  Here one thread owns a voxel of the raw grid,
// and the resampled tensors never exist: a member's value of a head is interpolated in registers from the few lines of
// its (much smaller) network grid that the voxel's taps touch, rounded to the member's dtype as the resampler would have
// stored it, and goes into the softmax / sigmoid of ensemble.hip.
//
// The result is bit for bit that of fnn_resample (order 1, order_z 0) / fnn_resample_torch per member followed by
// fnn_ensemble_export, so every value is formed by those kernels' expressions in their order: resample_default_common.h
// and resample_torch_common.h for the member's value (export_labels.hip says why the default family's clip is not
// needed), ensemble.hip's softmax in head order (max, then sum += expf(x - max) from 0), its average p_0 + p_1 + ... in
// member order, then / (float)N, and ensemble_common.h's merge rule.  A member whose grid is the cropped grid is read as
// it is, whatever its family: no weight-0 tap of its own value is formed (inf * 0 is NaN).
//
// Loop order: members outermost.  With heads outermost a thread would need the taps and weights of all 16 members live
// at once (16 x (8 offsets + 6 weights)), which spills.  So a member's taps and weights are computed once, its heads are
// walked three times (max, sum, probability - the second and third walk re-interpolate from lines that are still in
// cache), and head h's running sum over the members lives in LDS as acc[h * THREADS + tid]: written by member 0, added
// to by the others, which is the order of ensemble.hip; consecutive lanes are consecutive words, so no bank conflicts,
// and a thread only ever touches its own column, so no barrier.  A last walk over the heads divides, stores the average
// if asked, and applies the merge rule.  The host picks 256, 128 or 64 threads per block so that heads * THREADS * 4
// bytes fit the 160 KiB of a CU with as many threads resident as possible: 640 heads at most.
//
// A member's dtype, family and two-tap mask are uniform over the launch: one switch per member around a body templated
// like export_labels_*_kernel<T, M>, so that taps and weights stay in registers under compile-time indices.
// No atomics: the same input gives the same bytes.
#include "ensemble_common.h"
#include "output_common.h"
#include "resample_default_common.h"
#include "resample_torch_common.h"
#include "host_call.h"
#include <climits>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int ER_LDS_BYTES = 160 * 1024;
constexpr int ER_MIN_THREADS = 64, ER_MAX_THREADS = 256;
constexpr int ER_MAX_HEADS = ER_LDS_BYTES / (ER_MIN_THREADS * 4);            // 640

enum { ER_COPY = 0, ER_DEFAULT = 1, ER_TORCH = 2 };
// the body of a member: 0 / 1 copy fp16 / fp32, else 2 + ((kind - 1) * 2 + fp32) * 8 + two-tap mask
static constexpr int er_body(int kind, int f32, int mask) { return kind == ER_COPY ? f32 : 2 + ((kind - 1) * 2 + f32) * 8 + mask; }

struct ERMember {
    const void *p;             // [H][in0][in1][in2]
    long long in[3];
    double zoom[3];            // DGeo's
    float scale[3];            // RGeo's
    int sep;
    int body;
};

struct ERArgs {
    ERMember m[ENS_MAX_MEMBERS];
    int N, H;
    const int *order;          // regions_class_order on the device, or nullptr for plain labels
    CropBox box;
    float *avg;                // [H][o0][o1][o2] or nullptr
    void *labels;
    int label_u16;
};

// ---- a member's value of one head at cropped voxel c: value(p) with p the head's channel ------------------------------
template <typename T>
struct CopyTap {
    long long off;
    __device__ __forceinline__ CopyTap(const ERMember &, const CropBox &b, const long long (&c)[3]) {
        off = (c[0] * b.e[1] + c[1]) * b.e[2] + c[2];
    }
    __device__ __forceinline__ float value(const T *p) const { return (float)p[off]; }
};

template <typename T, int M>
struct DefaultTap {
    static constexpr int KM = ((M & 1) ? 4 : 0) | (M & 2) | ((M & 4) ? 1 : 0);       // the tap indices that are loaded
    long long off[8];
    double w[3][2];
    __device__ __forceinline__ DefaultTap(const ERMember &mb, const CropBox &b, const long long (&c)[3]) {
        DGeo g;
#pragma unroll
        for (int a = 0; a < 3; ++a) { g.in[a] = mb.in[a]; g.out[a] = b.e[a]; g.zoom[a] = mb.zoom[a]; }
        g.sep = mb.sep;
        long long i[3][2];
        d_axis<(M & 1) != 0>(g, 0, c[0], i[0], w[0]);
        d_axis<(M & 2) != 0>(g, 1, c[1], i[1], w[1]);
        d_axis<(M & 4) != 0>(g, 2, c[2], i[2], w[2]);
#pragma unroll
        for (int k = 0; k < 8; ++k) off[k] = (i[0][k >> 2] * g.in[1] + i[1][(k >> 1) & 1]) * g.in[2] + i[2][k & 1];
    }
    __device__ __forceinline__ float value(const T *p) const {
        T v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) if ((k & ~KM) == 0) v[k] = p[off[k]];
        return d_value<T, M>(v, w);
    }
};

template <typename T, int M>
struct TorchTap {
    static constexpr int KM = ((M & 1) ? 4 : 0) | (M & 2) | ((M & 4) ? 1 : 0);       // a corner outside it repeats corner k & KM
    Taps t;
    __device__ __forceinline__ TorchTap(const ERMember &mb, const CropBox &b, const long long (&c)[3]) {
        RGeo g;
#pragma unroll
        for (int a = 0; a < 3; ++a) { g.in[a] = mb.in[a]; g.out[a] = b.e[a]; g.scale[a] = mb.scale[a]; }
        g.sep = mb.sep;
        make_taps(g, c[0], c[1], c[2], t);
    }
    __device__ __forceinline__ float value(const T *p) const {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) if ((k & ~KM) == 0) v[k] = (float)p[t.off[k]];
#pragma unroll
        for (int k = 0; k < 8; ++k) if ((k & ~KM) != 0) v[k] = v[k & KM];
        return (float)store_cast<T>(blend(t, v));
    }
};

// ---- one member: its probabilities of this thread's voxel into acc[h * stride] (set by the first member, added to by the
// others), exactly as ensemble_export_kernel forms them
template <class TAP, typename T>
static __device__ __forceinline__ void member_pass(const ERMember &mb, const CropBox &box, const long long (&c)[3], int H,
                                                   bool regions, bool first, float *acc, int stride) {
    const TAP tap(mb, box, c);
    const long long nin = mb.in[0] * mb.in[1] * mb.in[2];
    const T *const base = (const T *)mb.p;
    const T *p = base;
    if (regions) {
#pragma unroll 4
        for (int h = 0; h < H; ++h, p += nin) {
            const float pr = 1.f / (1.f + expf(-tap.value(p)));
            acc[h * stride] = first ? pr : acc[h * stride] + pr;
        }
        return;
    }
    float mx = tap.value(p);
    p += nin;
#pragma unroll 4
    for (int h = 1; h < H; ++h, p += nin) mx = fmaxf(mx, tap.value(p));
    float sum = 0.f;
    p = base;
#pragma unroll 4
    for (int h = 0; h < H; ++h, p += nin) sum += expf(tap.value(p) - mx);
    p = base;
#pragma unroll 4
    for (int h = 0; h < H; ++h, p += nin) {
        const float pr = expf(tap.value(p) - mx) / sum;
        acc[h * stride] = first ? pr : acc[h * stride] + pr;
    }
}

#define ER_MASKS(base, TAP, T)                                                                       \
    case base + 0: member_pass<TAP<T, 0>, T>(mb, a.box, c, a.H, regions, first, acc, stride); break; \
    case base + 1: member_pass<TAP<T, 1>, T>(mb, a.box, c, a.H, regions, first, acc, stride); break; \
    case base + 2: member_pass<TAP<T, 2>, T>(mb, a.box, c, a.H, regions, first, acc, stride); break; \
    case base + 3: member_pass<TAP<T, 3>, T>(mb, a.box, c, a.H, regions, first, acc, stride); break; \
    case base + 4: member_pass<TAP<T, 4>, T>(mb, a.box, c, a.H, regions, first, acc, stride); break; \
    case base + 5: member_pass<TAP<T, 5>, T>(mb, a.box, c, a.H, regions, first, acc, stride); break; \
    case base + 6: member_pass<TAP<T, 6>, T>(mb, a.box, c, a.H, regions, first, acc, stride); break; \
    case base + 7: member_pass<TAP<T, 7>, T>(mb, a.box, c, a.H, regions, first, acc, stride); break;

// ---- N members' logits on their network grids -> average probabilities [H][o0][o1][o2] (optional) + labels [o0][o1][o2]
// on the raw grid.  Dynamic LDS: H * blockDim.x floats.
__global__ __launch_bounds__(ER_MAX_THREADS) void ensemble_resample_kernel(ERArgs a) {
    extern __shared__ float er_acc[];
    const long long n = a.box.o[0] * a.box.o[1] * a.box.o[2];
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long c[3];                                            // the voxel on the cropped grid
    const bool regions = a.order != nullptr;
    if (!crop_box_coords(a.box, i, c)) {
        // every member's probability is 1 for the background / 0 elsewhere, so the average is too, and both rules give label 0
        if (a.avg)
            for (int h = 0; h < a.H; ++h) a.avg[(size_t)h * n + i] = (!regions && h == 0) ? 1.f : 0.f;
        store_label(a.labels, a.label_u16, (size_t)i, 0);
        return;
    }
    const int stride = (int)blockDim.x;
    float *acc = er_acc + threadIdx.x;
    for (int m = 0; m < a.N; ++m) {
        const ERMember &mb = a.m[m];
        const bool first = m == 0;
        switch (mb.body) {                                     // uniform over the launch
            case 0: member_pass<CopyTap<f16>, f16>(mb, a.box, c, a.H, regions, first, acc, stride); break;
            case 1: member_pass<CopyTap<float>, float>(mb, a.box, c, a.H, regions, first, acc, stride); break;
            ER_MASKS(2, DefaultTap, f16)
            ER_MASKS(10, DefaultTap, float)
            ER_MASKS(18, TorchTap, f16)
            ER_MASKS(26, TorchTap, float)
            default: break;
        }
    }
    const float fn = (float)a.N;
    float best = -1.f;
    int label = 0;
    for (int h = 0; h < a.H; ++h) {
        const float v = acc[h * stride] / fn;
        if (a.avg) a.avg[(size_t)h * n + i] = v;
        ensemble_merge_rule(a.order, h, v, best, label);
    }
    store_label(a.labels, a.label_u16, (size_t)i, label);
}

#undef ER_MASKS

static_assert(er_body(ER_DEFAULT, 0, 0) == 2 && er_body(ER_DEFAULT, 1, 0) == 10 && er_body(ER_TORCH, 0, 0) == 18 &&
              er_body(ER_TORCH, 1, 7) == 33, "the switch of ensemble_resample_kernel follows er_body");

// threads per block: the most threads resident on a CU under its LDS (heads * threads * 4 bytes per block) and its 2048
// thread slots; the larger block among equals.  0: not even one block of 64 fits
static int er_threads(int heads) {
    int best = 0;
    long long best_resident = 0;
    for (int t = ER_MAX_THREADS; t >= ER_MIN_THREADS; t /= 2) {
        const long long lds = (long long)heads * t * 4;
        if (lds > ER_LDS_BYTES) continue;
        long long blocks = ER_LDS_BYTES / lds;
        if (blocks * t > 2048) blocks = 2048 / t;
        if (blocks * t > best_resident) { best_resident = blocks * t; best = t; }
    }
    return best;
}

}  // namespace

extern "C" int fnn_ensemble_resample_export(const fnn_ensemble_member *members, int n_members, int heads,
                                            const int32_t *regions_class_order, const int64_t bbox[6],
                                            const int64_t shape_before_cropping[3], const int32_t transpose_backward[3],
                                            float *avg_probs, void *labels, int label_dtype, void *stream) {
    static const char *const who = "fnn_ensemble_resample_export";
    if (!members || !bbox || !shape_before_cropping || !transpose_backward || !labels) return fnn_fail(FNN_E_INVALID, "NULL argument");
    if (n_members < 1 || n_members > ENS_MAX_MEMBERS) return fnn_fail(FNN_E_INVALID, "n_members must be 1..16");
    if (heads < 1) return fnn_fail(FNN_E_INVALID, "heads must be at least 1");
    if (int rc = fnn_check_label_dtype(label_dtype)) return rc;
    for (int m = 0; m < n_members; ++m) {
        const fnn_ensemble_member &mb = members[m];
        if (!mb.logits) return fnn_fail(FNN_E_INVALID, "NULL member logits");
        if (int rc = fnn_check_float_dtype(mb.dtype, "member logits dtype")) return rc;
        if (mb.family != FNN_RESAMPLE_DEFAULT && mb.family != FNN_RESAMPLE_TORCH) return fnn_fail(FNN_E_UNSUPPORTED, "unknown resampling family");
        if (mb.separate_axis < -1 || mb.separate_axis > 2) return fnn_fail(FNN_E_INVALID, "separate_axis must be -1 .. 2");
        for (int a = 0; a < 3; ++a) if (mb.shape[a] < 1) return fnn_fail(FNN_E_INVALID, "bad shape");
    }
    if (int rc = fnn_check_perm(transpose_backward, "transpose_backward")) return rc;
    ERArgs a{};
    if (int rc = crop_box_fill(a.box, bbox, shape_before_cropping, transpose_backward)) return rc;
    if (!regions_class_order && label_dtype == FNN_LABEL_U8 && heads > 256) return fnn_fail(FNN_E_INVALID, "more than 256 heads need uint16 labels");
    const int64_t extents[3] = {a.box.e[0], a.box.e[1], a.box.e[2]};
    for (int m = 0; m < n_members; ++m) {
        const fnn_ensemble_member &mb = members[m];
        const int64_t shape[4] = {heads, mb.shape[0], mb.shape[1], mb.shape[2]};
        RGeo rg{};                                             // the grid rule and its limits are the torch family's for both
        const char *why = "";
        if (int rc = rt_geometry(shape, extents, mb.separate_axis, rg, &why)) return fnn_fail(rc, why);
        ERMember &e = a.m[m];
        e.p = mb.logits; e.sep = mb.separate_axis;
        int mask = 0;
        bool same = true;
        for (int k = 0; k < 3; ++k) {
            e.in[k] = rg.in[k]; e.scale[k] = rg.scale[k]; e.zoom[k] = (double)rg.in[k] / (double)rg.out[k];
            same = same && rg.in[k] == rg.out[k];
            if (rg.in[k] != rg.out[k] && k != mb.separate_axis) mask |= 1 << k;
        }
        e.body = er_body(same ? ER_COPY : (mb.family == FNN_RESAMPLE_TORCH ? ER_TORCH : ER_DEFAULT), mb.dtype == FNN_OUT_F32, mask);
    }
    const int threads = heads <= ER_MAX_HEADS ? er_threads(heads) : 0;
    if (!threads) return fnn_failf(FNN_E_UNSUPPORTED, "more than %d heads: a voxel's running sums do not fit the LDS of a CU", ER_MAX_HEADS);
    const long long n = a.box.o[0] * a.box.o[1] * a.box.o[2];
    if ((n + threads - 1) / threads > UINT_MAX) return fnn_fail(FNN_E_UNSUPPORTED, "output grid too large");
    for (int m = 0; m < n_members; ++m)
        if (int rc = fnn_need_dev(who, {members[m].logits})) return rc;
    if (int rc = fnn_need_dev(who, {labels})) return rc;
    if (avg_probs)
        if (int rc = fnn_need_dev(who, {avg_probs})) return rc;
    a.N = n_members; a.H = heads; a.avg = avg_probs; a.labels = labels; a.label_u16 = label_dtype == FNN_LABEL_U16;
    HipCall call(stream);
    const DevBuf order = upload_order(regions_class_order, heads, call);
    a.order = order.as<int>();
    FnnOpKlog klog;                                            // the kernel's name for fnn_op_last_kernels
    fnn_allow_lds<ensemble_resample_kernel>();
    if (call.ok()) fnn_note_kernel("ensemble_resample_kernel");
    call.launch(ensemble_resample_kernel, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads),
                (size_t)heads * threads * 4, a);
    return call.finish();
}
