// prep.hip - whole-volume steps on either side of the sliding window, gfx950.
//
//   fnn_nonzero_bbox    crop_to_nonzero's bounding box (preprocessing/cropping/cropping.py:7-39)
//   fnn_preprocess      transpose_forward + crop + per-channel intensity normalisation
//                       (preprocessing/preprocessors/default_preprocessor.py:45-93 without the resampling call;
//                       preprocessing/normalization/default_normalization_schemes.py:27-109)
//   fnn_revert_labels   label map back to the uncropped, untransposed grid (inference/export_prediction.py:43-53)
//
// All three are HBM-bound element-wise / reduction kernels: one pass over the raw volume for the box, one pass
// for the statistics of the schemes that need them (two for ZScore: the mean, then the squared deviations about it),
// one read + one write for the result.
#include "host_call.h"
#include <cfloat>
#include <climits>
#include <cstdio>
#include <cmath>

extern "C" const char *fnn_last_error(const fnn_engine *e);

namespace {

struct PrepGeom {
    long long s[3];              // raw spatial shape
    int tf[3];                   // transposed axis a = raw axis tf[a]
    int C;
};

// ---- bounding box of the voxels where any channel is non-zero, in transposed coordinates
__global__ __launch_bounds__(256) void bbox_kernel(const float *raw, PrepGeom g, int *box /* lo[3], hi[3] (inclusive) */) {
    __shared__ int sbox[6];
    if (threadIdx.x < 3) sbox[threadIdx.x] = INT_MAX;
    else if (threadIdx.x < 6) sbox[threadIdx.x] = -1;
    __syncthreads();
    const long long n = g.s[0] * g.s[1] * g.s[2];
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        bool nz = false;
        for (int c = 0; c < g.C; ++c) nz |= raw[c * n + i] != 0.f;           // NaN != 0 is true, like numpy
        if (nz) {
            const int r[3] = {(int)(i / (g.s[1] * g.s[2])), (int)((i / g.s[2]) % g.s[1]), (int)(i % g.s[2])};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int t = r[g.tf[a]];
                lo[a] = t < lo[a] ? t : lo[a];
                hi[a] = t > hi[a] ? t : hi[a];
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (hi[a] >= 0) { atomicMin(&sbox[a], lo[a]); atomicMax(&sbox[3 + a], hi[a]); }
    }
    __syncthreads();
    if (threadIdx.x < 3) { if (sbox[threadIdx.x] != INT_MAX) atomicMin(&box[threadIdx.x], sbox[threadIdx.x]); }
    else if (threadIdx.x < 6) { if (sbox[threadIdx.x] >= 0) atomicMax(&box[threadIdx.x], sbox[threadIdx.x]); }
}

struct PrepParams {
    PrepGeom g;
    long long lo[3], ext[3];     // crop box in transposed coordinates: origin and extent
    int scheme[8];
    float a[8], b[8], lower[8], upper[8];     // per channel: out = (clip(x) - a) / b
    int use_mask[8];             // ZScore inside the filled non-zero mask only (use_mask_for_norm)
    const uint8_t *mask;         // [ext0][ext1][ext2]: 2 = outside, anything else = inside (or nullptr)
};

// raw offset of transposed-cropped voxel (t0, t1, t2)
static __device__ __forceinline__ long long raw_index(const PrepParams &p, long long t0, long long t1, long long t2) {
    long long r[3];
    r[p.g.tf[0]] = t0 + p.lo[0]; r[p.g.tf[1]] = t1 + p.lo[1]; r[p.g.tf[2]] = t2 + p.lo[2];
    return (r[0] * p.g.s[1] + r[1]) * p.g.s[2] + r[2];
}

// ---- per-channel statistics over the crop box: sum and sum of squares of (x - shift) (double), min, max.  ZScore runs it
// twice: shift = 0 for the mean, then shift = mean for the squared deviations - E[x^2] - mean^2 in one pass cancels on a
// channel that is nearly constant far from zero (mean 16384, std 0.002: what is left is rounding noise).  A NaN makes min and max NaN,
// like numpy's.
__global__ __launch_bounds__(256) void stats_kernel(const float *raw, PrepParams p, int c, double shift, double *sums /*[3]: sum, sumsq, count*/, unsigned *mm /*[2] ordered*/) {
    __shared__ double ssum[3][4];
    __shared__ unsigned smm[2];
    if (threadIdx.x == 0) { smm[0] = 0xffffffffu; smm[1] = 0u; }
    __syncthreads();
    const long long n = p.ext[0] * p.ext[1] * p.ext[2], nraw = p.g.s[0] * p.g.s[1] * p.g.s[2];
    double s1 = 0, s2 = 0, cnt = 0;
    float mn = FLT_MAX, mx = -FLT_MAX;
    bool any = false, nan = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long t2 = i % p.ext[2], t1 = (i / p.ext[2]) % p.ext[1], t0 = i / (p.ext[2] * p.ext[1]);
        const float v = raw[(long long)c * nraw + raw_index(p, t0, t1, t2)];
        if (p.use_mask[c] && p.mask[i] == 2) continue;          // outside the filled non-zero mask
        const double d = (double)v - shift;
        s1 += d; s2 += d * d; cnt += 1.0;
        mn = v < mn ? v : mn; mx = v > mx ? v : mx;
        nan |= v != v;
        any = true;
    }
    // order-preserving map float -> unsigned for the atomics; -NaN sorts below -inf and +NaN above +inf
    auto ord = [](float f) { unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); };
    if (nan) { mn = __uint_as_float(0xffc00000u); mx = __uint_as_float(0x7fc00000u); }
    if (any) { atomicMin(&smm[0], ord(mn)); atomicMax(&smm[1], ord(mx)); }
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); cnt += __shfl_down(cnt, off); }
    if ((threadIdx.x & 63) == 0) { ssum[0][threadIdx.x >> 6] = s1; ssum[1][threadIdx.x >> 6] = s2; ssum[2][threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsafeAtomicAdd(&sums[0], ssum[0][0] + ssum[0][1] + ssum[0][2] + ssum[0][3]);
        unsafeAtomicAdd(&sums[1], ssum[1][0] + ssum[1][1] + ssum[1][2] + ssum[1][3]);
        unsafeAtomicAdd(&sums[2], ssum[2][0] + ssum[2][1] + ssum[2][2] + ssum[2][3]);
        atomicMin(&mm[0], smm[0]); atomicMax(&mm[1], smm[1]);
    }
}

// ---- create_nonzero_mask (cropping.py:7-17) inside the crop box: 0 = some channel non-zero, 1 = background, and the
// background voxels on the box faces start as 2 = outside.  binary_fill_holes == "background that cannot reach the
// border through 6-connected background stays inside"; restricting it to the box is exact because everything beyond
// a box face that is not the image border is background connected to the image border.
__global__ __launch_bounds__(256) void mask_init_kernel(const float *raw, PrepParams p, uint8_t *m) {
    const long long n = p.ext[0] * p.ext[1] * p.ext[2], nraw = p.g.s[0] * p.g.s[1] * p.g.s[2];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long t2 = i % p.ext[2], t1 = (i / p.ext[2]) % p.ext[1], t0 = i / (p.ext[2] * p.ext[1]);
    const long long r = raw_index(p, t0, t1, t2);
    bool nz = false;
    for (int c = 0; c < p.g.C; ++c) nz |= raw[(long long)c * nraw + r] != 0.f;
    const bool face = t0 == 0 || t1 == 0 || t2 == 0 || t0 == p.ext[0] - 1 || t1 == p.ext[1] - 1 || t2 == p.ext[2] - 1;
    m[i] = nz ? 0 : (face ? 2 : 1);
}

// One sweep: every thread owns `seg` voxels of a line along `axis` (the whole line when the box has lines enough to fill
// the device) and carries "outside" forwards and backwards through runs of background, starting from the voxel before /
// behind its segment; a voxel also turns outside when a neighbour on another line already is (checked along the way).
// A sweep that changes nothing has looked at all six neighbours of every background voxel, whatever `seg` is.
__global__ __launch_bounds__(256) void mask_sweep_kernel(PrepParams p, int axis, long long seg, uint8_t *m, int *changed) {
    const long long e[3] = {p.ext[0], p.ext[1], p.ext[2]};
    const int a1 = axis == 0 ? 1 : 0, a2 = axis == 2 ? 1 : 2;
    const long long lines = e[a1] * e[a2];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long l = t % lines, k0 = (t / lines) * seg;
    if (k0 >= e[axis]) return;
    const long long k1 = k0 + seg < e[axis] ? k0 + seg : e[axis];
    const long long c1 = l / e[a2], c2 = l % e[a2];
    const long long st[3] = {e[1] * e[2], e[2], 1};
    const long long base = c1 * st[a1] + c2 * st[a2];
    bool any = false;
    for (int dir = 0; dir < 2; ++dir) {
        bool carry = dir ? (k1 < e[axis] && m[base + k1 * st[axis]] == 2) : (k0 > 0 && m[base + (k0 - 1) * st[axis]] == 2);
        for (long long k = k0; k < k1; ++k) {
            const long long pos = dir ? k1 - 1 - (k - k0) : k;
            const long long i = base + pos * st[axis];
            uint8_t v = m[i];
            if (v == 1) {
                bool out = carry;
                if (!out) {                                   // side neighbours on the two other axes
                    if (c1 > 0) out |= m[i - st[a1]] == 2;
                    if (c1 < e[a1] - 1) out |= m[i + st[a1]] == 2;
                    if (c2 > 0) out |= m[i - st[a2]] == 2;
                    if (c2 < e[a2] - 1) out |= m[i + st[a2]] == 2;
                }
                if (out) { m[i] = 2; v = 2; any = true; }
            }
            carry = v == 2;
        }
    }
    if (any) *changed = 1;
}

// ---- out[c][t0][t1][t2] = normalise_c(raw[c][transposed, cropped])
__global__ __launch_bounds__(256) void apply_kernel(const float *raw, PrepParams p, float *out) {
    const long long n = p.ext[0] * p.ext[1] * p.ext[2], nraw = p.g.s[0] * p.g.s[1] * p.g.s[2];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * p.g.C) return;
    const int c = (int)(i / n);
    const long long j = i - (long long)c * n;
    const long long t2 = j % p.ext[2], t1 = (j / p.ext[2]) % p.ext[1], t0 = j / (p.ext[2] * p.ext[1]);
    float v = raw[(long long)c * nraw + raw_index(p, t0, t1, t2)];
    switch (p.scheme[c]) {
    case FNN_NORM_CT:                       // np.clip, -= mean, /= max(std, 1e-8): three fp32 roundings
        v = v < p.lower[c] ? p.lower[c] : (v > p.upper[c] ? p.upper[c] : v);      // NaN stays NaN like np.clip
        v = __fdiv_rn(__fsub_rn(v, p.a[c]), p.b[c]);
        break;
    case FNN_NORM_ZSCORE:                   // image[mask] = (image[mask] - mean) / max(std, 1e-8): outside stays as it is
        if (!(p.use_mask[c] && p.mask[j] == 2)) v = __fdiv_rn(__fsub_rn(v, p.a[c]), p.b[c]);
        break;
    case FNN_NORM_RESCALE01:
        v = __fdiv_rn(__fsub_rn(v, p.a[c]), p.b[c]);
        break;
    case FNN_NORM_RGB01:
        v = __fdiv_rn(v, 255.f);
        break;
    default: break;
    }
    out[i] = v;
}

// ---- labels [b0][b1][b2] (transposed, cropped) -> out [s0][s1][s2] in the original axis order
template <typename LT>
__global__ __launch_bounds__(256) void revert_kernel(const LT *seg, CropBox b, LT *out) {
    const long long n = b.o[0] * b.o[1] * b.o[2];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    size_t v;
    out[i] = crop_box_voxel(b, i, v) ? seg[v] : (LT)0;
}

// ---- logits [H][b0][b1][b2] (transposed, cropped grid) -> probabilities [H][s0][s1][s2] + labels [s0][s1][s2] on the
// original grid: apply_inference_nonlin (fp32 softmax over the heads / sigmoid for regions), the label rule on the
// probabilities, both reverted croppings (background probability 1 outside the box for plain labels), transposes back.
// expf / the division follow the device's fp32 library: probabilities agree with torch's CPU softmax to ~1e-7.
template <typename IT, typename LT>
__global__ __launch_bounds__(256) void export_prob_kernel(const IT *logits, int H, const int *order, CropBox b, float *probs,
                                                          LT *labels) {
    const long long n = b.o[0] * b.o[1] * b.o[2];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    size_t v;
    if (!crop_box_voxel(b, i, v)) {
        for (int h = 0; h < H; ++h) probs[(size_t)h * n + i] = (!order && h == 0) ? 1.f : 0.f;
        labels[i] = 0;
        return;
    }
    const size_t plane = (size_t)b.e[0] * b.e[1] * b.e[2];
    if (order) {
        int seg = 0;
        for (int h = 0; h < H; ++h) {
            const float x = (float)logits[h * plane + v];
            const float pr = 1.f / (1.f + expf(-x));
            probs[(size_t)h * n + i] = pr;
            if (pr > 0.5f) seg = order[h];
        }
        labels[i] = (LT)seg;
        return;
    }
    float mx = (float)logits[v];
    for (int h = 1; h < H; ++h) mx = fmaxf(mx, (float)logits[h * plane + v]);
    float sum = 0.f;
    for (int h = 0; h < H; ++h) sum += expf((float)logits[h * plane + v] - mx);
    float best = -1.f; int arg = 0;
    for (int h = 0; h < H; ++h) {
        const float pr = expf((float)logits[h * plane + v] - mx) / sum;
        probs[(size_t)h * n + i] = pr;
        if (pr > best) { best = pr; arg = h; }                   // first maximum wins (numpy / torch argmax)
    }
    labels[i] = (LT)arg;
}

// ---- seg = where(binary_fill_holes(nonzero_mask), 0, -1) of crop_to_nonzero (cropping.py:19-39), as a byte map of the n
// voxels of the crop box.  FNN_OK also when a HIP call failed: that stays in the call's status
static int fill_holes_mask(const float *raw, const PrepParams &p, long long n, uint8_t *mask, HipCall &call) {
    DevBuf changed;
    if (!changed.alloc(sizeof(int))) return fnn_fail(FNN_E_HIP, "hipMalloc failed");
    call.launch(mask_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, raw, p, mask);
    // Iterations until one changes nothing.  Each one before it turns at least one voxel outside, so no box takes more
    // than n + 1 (a corridor that winds through a thin box does take thousands): running out of them is an error,
    // never a mask that is silently wrong.
    bool converged = false;
    for (long long iter = 0; iter <= n && call.ok() && !converged; ++iter) {
        int h = 0;
        call.copy(changed.p, &h, sizeof(int), hipMemcpyHostToDevice);
        for (int axis = 0; axis < 3; ++axis) {
            // a thread per line where that makes 64 Ki threads, else the lines cut into segments of 32 voxels or more
            const long long lines = n / p.ext[axis];
            const long long cuts = lines >= 65536 ? 1 : (65536 + lines - 1) / lines;
            long long seg = (p.ext[axis] + cuts - 1) / cuts;
            seg = seg < 32 ? 32 : seg;
            const long long threads = lines * ((p.ext[axis] + seg - 1) / seg);
            call.launch(mask_sweep_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, p, axis, seg, mask, changed.as<int>());
        }
        call.copy(&h, changed.p, sizeof(int), hipMemcpyDeviceToHost);
        converged = call.sync() && !h;
    }
    if (call.ok() && !converged) return fnn_fail(FNN_E_HIP, "the fill-holes sweeps of the non-zero mask did not converge");
    return FNN_OK;
}

// ---- ZScore / RescaleTo01: the statistics of channel c over the crop box -> p.a[c], p.b[c].  sc: 5 doubles of device
// scratch (sum, sum of squares, count | min, max as ordered unsigned)
static void channel_stats(const float *raw, PrepParams &p, int c, long long n, double *sc, HipCall &call) {
    unsigned *mm = (unsigned *)(sc + 3);
    const double z[3] = {0, 0, 0};
    const unsigned mi[2] = {0xffffffffu, 0u};
    double hs[3]; unsigned hm[2];
    long long blocks = (n + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    auto pass = [&](double shift) {
        call.copy(sc, z, sizeof(z), hipMemcpyHostToDevice);
        call.launch(stats_kernel, dim3((unsigned)blocks), dim3(256), 0, raw, p, c, shift, sc, mm);
        call.copy(hs, sc, sizeof(hs), hipMemcpyDeviceToHost);
    };
    call.copy(mm, mi, sizeof(mi), hipMemcpyHostToDevice);
    pass(0.0);
    call.copy(hm, mm, sizeof(hm), hipMemcpyDeviceToHost);
    if (!call.sync()) return;
    if (p.scheme[c] == FNN_NORM_ZSCORE) {
        const double cntd = hs[2] > 0 ? hs[2] : 1.0;             // voxels inside the mask (all of them without one)
        const double mean = hs[0] / cntd;
        // second pass: the squared deviations about the mean (and the sum of the deviations, which takes out
        // what the rounding of the mean left in)
        pass(mean);
        if (!call.sync()) return;
        const double dev = hs[0] / cntd;
        double var = hs[1] / cntd - dev * dev;
        var = var < 0 ? 0 : var;                                      // NaN stays NaN, like numpy's std
        const float stdf = (float)sqrt(var);
        p.a[c] = (float)mean; p.b[c] = 1e-8f > stdf ? 1e-8f : stdf;   // python's max(std, 1e-8): a NaN std stays
    } else {
        auto unord = [](unsigned u) { u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u; return __builtin_bit_cast(float, u); };
        const float mn = unord(hm[0]), mx = unord(hm[1]);
        const float range = mx - mn;                                   // = (image - image.min()).max() in fp32
        p.a[c] = mn; p.b[c] = range < 1e-8f ? 1e-8f : range;            // np.clip(max, 1e-8, None): NaN stays NaN
    }
}

}  // namespace

extern "C" {

int fnn_nonzero_bbox(const float *raw, const int64_t shape[4], const int32_t transpose_forward[3], int64_t bbox[6], void *stream) {
    if (!raw || !shape || !transpose_forward || !bbox) return fnn_fail(FNN_E_INVALID, "NULL argument");
    if (int rc = fnn_check_perm(transpose_forward, "transpose_forward")) return rc;
    if (shape[0] < 1 || shape[0] > 8 || shape[1] < 1 || shape[2] < 1 || shape[3] < 1) return fnn_fail(FNN_E_INVALID, "bad shape (1..8 channels)");
    if (int rc = fnn_need_dev("fnn_nonzero_bbox", {raw}, "a device pointer")) return rc;
    PrepGeom g{};
    for (int d = 0; d < 3; ++d) { g.s[d] = shape[1 + d]; g.tf[d] = transpose_forward[d]; }
    g.C = (int)shape[0];
    DevBuf box;
    if (!box.alloc(6 * sizeof(int))) return fnn_fail(FNN_E_HIP, "hipMalloc failed");
    const int init[6] = {INT_MAX, INT_MAX, INT_MAX, -1, -1, -1};
    int h[6];
    const long long n = g.s[0] * g.s[1] * g.s[2];
    long long blocks = (n + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    HipCall call(stream);
    call.copy(box.p, init, sizeof(init), hipMemcpyHostToDevice);
    call.launch(bbox_kernel, dim3((unsigned)blocks), dim3(256), 0, raw, g, box.as<int>());
    call.copy(h, box.p, sizeof(h), hipMemcpyDeviceToHost);
    if (!call.sync()) return call.fail();
    for (int a = 0; a < 3; ++a) {
        if (h[3 + a] < 0) { bbox[2 * a] = 0; bbox[2 * a + 1] = shape[1 + transpose_forward[a]]; }   // empty mask: the full extent
        else { bbox[2 * a] = h[a]; bbox[2 * a + 1] = h[3 + a] + 1; }
    }
    return FNN_OK;
}

int fnn_preprocess(const float *raw, const int64_t shape[4], const int32_t transpose_forward[3], const int64_t bbox[6],
                   const fnn_norm_desc *norm, float *out, void *stream) {
    if (!raw || !shape || !transpose_forward || !bbox || !norm || !out) return fnn_fail(FNN_E_INVALID, "NULL argument");
    if (int rc = fnn_check_perm(transpose_forward, "transpose_forward")) return rc;
    if (shape[0] < 1 || shape[0] > 8) return fnn_fail(FNN_E_INVALID, "1..8 channels");
    if (int rc = fnn_need_dev("fnn_preprocess", {raw, out})) return rc;
    PrepParams p{};
    int64_t transposed[3];
    for (int d = 0; d < 3; ++d) { p.g.s[d] = shape[1 + d]; p.g.tf[d] = transpose_forward[d]; transposed[d] = shape[1 + transpose_forward[d]]; }
    p.g.C = (int)shape[0];
    CropBox box{};
    if (int rc = crop_box_fill(box, bbox, transposed, nullptr, "bbox outside the (transposed) image")) return rc;
    for (int a = 0; a < 3; ++a) { p.lo[a] = box.lo[a]; p.ext[a] = box.e[a]; }
    // every channel's scheme before the first device call: an unknown one is refused with nothing run.  The mask and
    // statistics kernels therefore see scheme / lower / upper (and CT's a, b) of all channels filled in; they read use_mask,
    // mask and the shape only, and must not come to rely on the rest either way
    bool want_mask = false;
    for (int c = 0; c < p.g.C; ++c) {
        const fnn_norm_desc &d = norm[c];
        if (d.scheme != FNN_NORM_NONE && d.scheme != FNN_NORM_ZSCORE && d.scheme != FNN_NORM_CT && d.scheme != FNN_NORM_RESCALE01 &&
            d.scheme != FNN_NORM_RGB01)
            return fnn_fail(FNN_E_UNSUPPORTED, "unknown normalisation scheme");
        p.scheme[c] = d.scheme;
        p.a[c] = 0.f; p.b[c] = 1.f; p.lower[c] = d.lower; p.upper[c] = d.upper;
        if (d.scheme == FNN_NORM_CT) { p.a[c] = d.mean; p.b[c] = d.std > 1e-8f ? d.std : 1e-8f; }   // max(std_intensity, 1e-8)
        p.use_mask[c] = d.scheme == FNN_NORM_ZSCORE && d.use_mask;
        want_mask |= p.use_mask[c] != 0;
    }
    const long long n = p.ext[0] * p.ext[1] * p.ext[2];
    DevBuf sums, mask;
    if (!sums.alloc(8 * 5 * sizeof(double)) || (want_mask && !mask.alloc((size_t)n))) return fnn_fail(FNN_E_HIP, "hipMalloc failed");
    HipCall call(stream);
    if (want_mask) {
        if (int rc = fill_holes_mask(raw, p, n, mask.as<uint8_t>(), call)) return rc;
        p.mask = mask.as<uint8_t>();
    }
    for (int c = 0; c < p.g.C; ++c)
        if (p.scheme[c] == FNN_NORM_ZSCORE || p.scheme[c] == FNN_NORM_RESCALE01) channel_stats(raw, p, c, n, sums.as<double>() + c * 5, call);
    call.launch(apply_kernel, dim3((unsigned)((n * p.g.C + 255) / 256)), dim3(256), 0, raw, p, out);
    return call.finish();
}

int fnn_revert_labels(const void *seg, int label_dtype, const int64_t bbox[6], const int64_t shape_before_cropping[3],
                      const int32_t transpose_backward[3], void *out, void *stream) {
    if (!seg || !bbox || !shape_before_cropping || !transpose_backward || !out) return fnn_fail(FNN_E_INVALID, "NULL argument");
    if (int rc = fnn_check_perm(transpose_backward, "transpose_backward")) return rc;
    if (int rc = fnn_check_label_dtype(label_dtype)) return rc;
    if (int rc = fnn_need_dev("fnn_revert_labels", {seg, out})) return rc;
    CropBox box{};
    if (int rc = crop_box_fill(box, bbox, shape_before_cropping, transpose_backward)) return rc;
    const long long n = box.o[0] * box.o[1] * box.o[2];
    HipCall call(stream);
    fnn_by_label(label_dtype, [&](auto lt) {
        using LT = decltype(lt);
        call.launch(revert_kernel<LT>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const LT *)seg, box, (LT *)out);
    });
    return call.finish();
}

int fnn_export_probabilities(const void *logits, int logits_dtype, int heads, const int32_t *regions_class_order,
                             const int64_t bbox[6], const int64_t shape_before_cropping[3],
                             const int32_t transpose_backward[3], float *probs, void *labels, int label_dtype, void *stream) {
    if (!logits || !bbox || !shape_before_cropping || !transpose_backward || !probs || !labels) return fnn_fail(FNN_E_INVALID, "NULL argument");
    if (int rc = fnn_check_perm(transpose_backward, "transpose_backward")) return rc;
    if (int rc = fnn_check_label_dtype(label_dtype)) return rc;
    if (int rc = fnn_check_float_dtype(logits_dtype, "logits dtype")) return rc;
    if (heads < 1 || heads > 4096) return fnn_fail(FNN_E_INVALID, "bad number of heads");
    if (int rc = fnn_need_dev("fnn_export_probabilities", {logits, probs, labels})) return rc;
    CropBox box{};
    if (int rc = crop_box_fill(box, bbox, shape_before_cropping, transpose_backward)) return rc;
    const long long n = box.o[0] * box.o[1] * box.o[2];
    HipCall call(stream);
    const DevBuf order = upload_order(regions_class_order, heads, call);
    if (regions_class_order && !order.p) return fnn_fail(FNN_E_HIP, "hipMalloc failed");
    fnn_by_float(logits_dtype, [&](auto it) {
        fnn_by_label(label_dtype, [&](auto lt) {
            using IT = decltype(it);
            using LT = decltype(lt);
            call.launch(export_prob_kernel<IT, LT>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const IT *)logits, heads,
                        order.as<int>(), box, probs, (LT *)labels);
        });
    });
    return call.finish();
}

}  // extern "C"
