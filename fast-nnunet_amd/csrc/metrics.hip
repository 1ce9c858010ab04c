// metrics.hip - exact confusion counts of label maps for nnU-Net's evaluation, gfx950.
//
//   fnn_confusion_counts   compute_tp_fp_fn_tn (evaluation/evaluate_predictions.py:76-85) for every label of a
//                          dataset at once: the [reference class][predicted class] matrix of 1..4 predictions
//
// One launch per band of reference rows.  Each workgroup keeps the band's matrix of every prediction as a u32 histogram
// in LDS, streams its share of the maps in 16-byte chunks (ref read once for all predictions) and flushes each non-zero
// bin with one 64-bit global atomic add.  Three guards keep hot bins off the LDS atomics:
//   - a chunk whose 16 bytes of ref are one value and whose prediction chunk equals it counts as one add of 8 or 16;
//   - each thread aggregates runs of one (ref, pred) bin per prediction in registers and adds the run when it ends;
//   - the ("other", "other") bin - background in nnU-Net's use - is never counted: the host derives it from the
//     number of counted voxels, which each workgroup adds once.
// Integers only: the result does not depend on scheduling.
#include "host_call.h"
#include <climits>
#include <vector>

namespace {

constexpr int CM_THREADS = 512;
constexpr int CM_MAX_PRED = 4;
constexpr int CM_MAX_CLASSES = 255;        // + "other": class indices fit a byte
constexpr int CM_TABLE_LDS = 4096;         // label values looked up in LDS; a longer table is read from global memory
constexpr int CM_BINS = 15104;             // u32 bins per workgroup: 59 KiB + the 4 KiB table, under 64 KiB
constexpr long long CM_MAX_WG_VOX = 1ll << 30;   // voxels per workgroup: every u32 bin and counter stays exact

struct CMArgs {
    const void *ref;
    const void *pred[CM_MAX_PRED];
    long long n_chunks;                    // whole 16-byte chunks
    long long n_vox;
    const unsigned char *gtable;           // class of each value (other = n_classes), n_table entries
    int n_table;
    int n_classes;                         // "other" is class n_classes
    int ignore;                            // -1: none
    int row_lo, rows;                      // this band: reference classes row_lo .. row_lo + rows - 1
    unsigned long long *counts;            // [n_pred][n_classes + 1][n_classes + 1]
    unsigned long long *counted;           // voxels not ignored (band 0 only)
};

template <typename T, int NP>
struct Counter {
    unsigned int *hist;                    // LDS [NP][rows][n_classes + 1]
    const unsigned char *ltab;             // LDS table (CM_TABLE_LDS entries) or nullptr
    const unsigned char *gtab;
    int n_table, other, cols, row_lo, rows, ignore;
    int cur[NP];
    unsigned int cnt[NP];
    unsigned int counted;

    __device__ __forceinline__ int cls(int v) const {
        if (v >= n_table) return other;
        return ltab ? ltab[v] : gtab[v];
    }
    __device__ __forceinline__ void add(int p, int rc, int pc, unsigned int k) {
        if (rc == other && pc == other) return;                 // derived on the host
        const int r = rc - row_lo;
        if ((unsigned)r >= (unsigned)rows) return;              // another band
        const int bin = (p * rows + r) * cols + pc;
        if (bin == cur[p]) { cnt[p] += k; return; }
        if (cur[p] >= 0) atomicAdd(hist + cur[p], cnt[p]);
        cur[p] = bin;
        cnt[p] = k;
    }
    __device__ __forceinline__ void flush() {
#pragma unroll
        for (int p = 0; p < NP; ++p)
            if (cur[p] >= 0) atomicAdd(hist + cur[p], cnt[p]);
    }
};

constexpr int per_chunk(int bytes) { return 16 / bytes; }

template <typename T>
__device__ __forceinline__ int elem(const uint4 &c, int k) {
    const unsigned int w = (&c.x)[k * (int)sizeof(T) / 4];
    if (sizeof(T) == 1) return (w >> (8 * (k & 3))) & 0xff;
    return (w >> (16 * (k & 1))) & 0xffff;
}

template <typename T>
__device__ __forceinline__ bool uniform(const uint4 &c) {
    const unsigned int splat = sizeof(T) == 1 ? (c.x & 0xff) * 0x01010101u : (c.x & 0xffff) * 0x00010001u;
    return c.x == splat && c.y == splat && c.z == splat && c.w == splat;
}

__device__ __forceinline__ bool same(const uint4 &a, const uint4 &b) {
    return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
}

// one chunk of VPC voxels: ref chunk r, prediction chunks q[0..NP)
template <typename T, int NP>
__device__ __forceinline__ void count_chunk(Counter<T, NP> &c, const uint4 &r, const uint4 *q) {
    constexpr int VPC = per_chunk(sizeof(T));
    if (uniform<T>(r)) {
        const int rv = elem<T>(r, 0);
        if (rv == c.ignore) return;
        c.counted += VPC;
        const int rc = c.cls(rv);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (same(q[p], r)) { c.add(p, rc, rc, VPC); continue; }
#pragma unroll
            for (int k = 0; k < VPC; ++k) c.add(p, rc, c.cls(elem<T>(q[p], k)), 1);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < VPC; ++k) {
        const int rv = elem<T>(r, k);
        if (rv == c.ignore) continue;
        ++c.counted;
        const int rc = c.cls(rv);
#pragma unroll
        for (int p = 0; p < NP; ++p) c.add(p, rc, c.cls(elem<T>(q[p], k)), 1);
    }
}

template <typename T, int NP>
__global__ __launch_bounds__(CM_THREADS) void cm_count_kernel(CMArgs a) {
    __shared__ unsigned int hist[CM_BINS];
    __shared__ unsigned char ltab[CM_TABLE_LDS];
    __shared__ unsigned int wg_counted;
    const int cols = a.n_classes + 1;
    const int nbins = NP * a.rows * cols;
    const bool lds_table = a.n_table <= CM_TABLE_LDS;
    for (int k = threadIdx.x; k < nbins; k += CM_THREADS) hist[k] = 0;
    if (lds_table)
        for (int k = threadIdx.x; k < a.n_table; k += CM_THREADS) ltab[k] = a.gtable[k];
    if (threadIdx.x == 0) wg_counted = 0;
    __syncthreads();

    Counter<T, NP> c;
    c.hist = hist;
    c.ltab = lds_table ? ltab : nullptr;
    c.gtab = a.gtable;
    c.n_table = a.n_table;
    c.other = a.n_classes;
    c.cols = cols;
    c.row_lo = a.row_lo;
    c.rows = a.rows;
    c.ignore = a.ignore;
    c.counted = 0;
#pragma unroll
    for (int p = 0; p < NP; ++p) { c.cur[p] = -1; c.cnt[p] = 0; }

    const uint4 *ref = (const uint4 *)a.ref;
    const uint4 *pred[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) pred[p] = (const uint4 *)a.pred[p];
    const long long stride = (long long)gridDim.x * CM_THREADS;
    for (long long i = (long long)blockIdx.x * CM_THREADS + threadIdx.x; i < a.n_chunks; i += stride) {
        const uint4 r = ref[i];
        uint4 q[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) q[p] = pred[p][i];
        count_chunk<T, NP>(c, r, q);
    }
    // the voxels after the last whole chunk: one per thread of workgroup 0
    constexpr int VPC = per_chunk(sizeof(T));
    if (blockIdx.x == 0) {
        const long long v = a.n_chunks * VPC + threadIdx.x;
        if (threadIdx.x < VPC && v < a.n_vox) {
            const int rv = ((const T *)a.ref)[v];
            if (rv != c.ignore) {
                ++c.counted;
                const int rc = c.cls(rv);
#pragma unroll
                for (int p = 0; p < NP; ++p) c.add(p, rc, c.cls(((const T *)a.pred[p])[v]), 1);
            }
        }
    }
    c.flush();
    if (a.row_lo == 0) {
        unsigned int s = c.counted;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&wg_counted, s);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nbins; k += CM_THREADS) {
        const unsigned int v = hist[k];
        if (!v) continue;
        const int p = k / (a.rows * cols), rem = k - p * a.rows * cols;
        const int row = a.row_lo + rem / cols, col = rem % cols;
        atomicAdd(a.counts + ((size_t)p * cols + row) * cols + col, (unsigned long long)v);
    }
    if (threadIdx.x == 0 && a.row_lo == 0 && wg_counted) atomicAdd(a.counted, (unsigned long long)wg_counted);
}

template <typename T>
void launch_np(int n_pred, dim3 grid, const CMArgs &a, HipCall &call) {
    switch (n_pred) {
    case 1: call.launch(cm_count_kernel<T, 1>, grid, dim3(CM_THREADS), 0, a); break;
    case 2: call.launch(cm_count_kernel<T, 2>, grid, dim3(CM_THREADS), 0, a); break;
    case 3: call.launch(cm_count_kernel<T, 3>, grid, dim3(CM_THREADS), 0, a); break;
    default: call.launch(cm_count_kernel<T, 4>, grid, dim3(CM_THREADS), 0, a); break;
    }
}

}  // namespace

extern "C" {

int fnn_confusion_counts(const void *ref, const void *const *pred, int n_pred, int label_dtype, int64_t n_vox,
                         const int32_t *class_of_value, int n_table, int n_classes, int ignore_value, int64_t *counts,
                         void *stream) {
    if (int rc = fnn_check_label_dtype(label_dtype)) return rc;
    if (n_pred < 1 || n_pred > CM_MAX_PRED) return fnn_fail(FNN_E_INVALID, "fnn_confusion_counts: n_pred must be 1..4");
    if (n_classes < 0 || n_classes > CM_MAX_CLASSES) return fnn_fail(FNN_E_INVALID, "fnn_confusion_counts: n_classes must be 0..255");
    if (n_vox < 0) return fnn_fail(FNN_E_INVALID, "negative voxel count");
    if (n_table < 0 || (n_table > 0 && !class_of_value)) return fnn_fail(FNN_E_INVALID, "bad class table");
    if (!counts || !pred) return fnn_fail(FNN_E_INVALID, "NULL pred or counts");
    for (int v = 0; v < n_table; ++v)
        if (class_of_value[v] < -1 || class_of_value[v] >= n_classes)
            return fnn_fail(FNN_E_INVALID, "class_of_value entry outside [-1, n_classes)");
    const int cols = n_classes + 1;
    const size_t n_counts = (size_t)n_pred * cols * cols;
    for (size_t k = 0; k < n_counts; ++k) counts[k] = 0;
    if (n_vox == 0) return FNN_OK;
    const size_t esize = label_dtype == FNN_LABEL_U16 ? 2 : 1;
    const int max_value = label_dtype == FNN_LABEL_U16 ? 65535 : 255;
    for (int p = -1; p < n_pred; ++p) {                              // the reference map, then every prediction
        const void *map = p < 0 ? ref : pred[p];
        if (int rc = fnn_need_dev("fnn_confusion_counts", {map}, "device label maps")) return rc;
        if ((uintptr_t)map & 15) return fnn_fail(FNN_E_INVALID, "fnn_confusion_counts: label maps must be 16-byte aligned");
    }

    // the table the kernel reads: values the dtype cannot hold dropped, trailing "other" entries trimmed
    int n_tab = n_table < max_value + 1 ? n_table : max_value + 1;
    while (n_tab > 0 && class_of_value[n_tab - 1] < 0) --n_tab;
    std::vector<unsigned char> htab((size_t)(n_tab > 0 ? n_tab : 1));
    for (int v = 0; v < n_tab; ++v) htab[v] = (unsigned char)(class_of_value[v] < 0 ? n_classes : class_of_value[v]);

    // reference rows per launch: the whole matrix when it fits the LDS histogram, else bands of rows
    const int rows_fit = CM_BINS / (n_pred * cols);
    const int band = rows_fit < cols ? rows_fit : cols;

    int dev = 0, cus = 0;
    hipError_t r = hipGetDevice(&dev);
    if (r == hipSuccess) r = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (r != hipSuccess) { (void)hipGetLastError(); return fnn_fail(FNN_E_HIP, hipGetErrorString(r)); }
    const long long per_chunk_vox = (long long)(16 / esize);
    const long long n_chunks = n_vox / per_chunk_vox;
    long long blocks = (n_chunks + CM_THREADS - 1) / CM_THREADS;
    const long long resident = 2ll * (cus > 0 ? cus : 1);           // two 64 KiB workgroups per CU
    if (blocks > resident) blocks = resident;
    const long long need = (n_vox + CM_MAX_WG_VOX - 1) / CM_MAX_WG_VOX;
    if (blocks < need) blocks = need;
    if (blocks < 1) blocks = 1;
    if (blocks > INT_MAX) return fnn_fail(FNN_E_UNSUPPORTED, "fnn_confusion_counts: volume too large");

    // scratch: counts [n_counts] u64 | counted u64 | table [n_tab] u8
    const size_t off_table = (n_counts + 1) * 8;
    DevBuf scratch;
    if (!scratch.alloc(off_table + htab.size())) return fnn_fail(FNN_E_HIP, "hipMalloc failed (confusion counts)");
    unsigned long long *dcounts = scratch.as<unsigned long long>();
    HipCall call(stream);
    call.fill(scratch.p, 0, off_table);
    if (n_tab > 0) call.copy(scratch.as<char>(off_table), htab.data(), (size_t)n_tab, hipMemcpyHostToDevice);

    CMArgs a{};
    a.ref = ref;
    for (int p = 0; p < n_pred; ++p) a.pred[p] = pred[p];
    a.n_chunks = n_chunks;
    a.n_vox = n_vox;
    a.gtable = scratch.as<unsigned char>(off_table);
    a.n_table = n_tab;
    a.n_classes = n_classes;
    a.ignore = ignore_value >= 0 && ignore_value <= max_value ? ignore_value : -1;
    a.counts = dcounts;
    a.counted = dcounts + n_counts;
    for (int lo = 0; lo < cols; lo += band) {
        a.row_lo = lo;
        a.rows = cols - lo < band ? cols - lo : band;
        fnn_by_label(label_dtype, [&](auto lt) { launch_np<decltype(lt)>(n_pred, dim3((unsigned)blocks), a, call); });
    }
    call.copy(counts, dcounts, n_counts * 8, hipMemcpyDeviceToHost);
    unsigned long long counted = 0;
    call.copy(&counted, dcounts + n_counts, 8, hipMemcpyDeviceToHost);
    call.sync();
    scratch.free();
    if (!call.ok()) return call.fail();
    // the ("other", "other") bin of every prediction: counted voxels minus every other bin
    const size_t oo = (size_t)n_classes * cols + n_classes;
    for (int p = 0; p < n_pred; ++p) {
        int64_t *m = counts + (size_t)p * cols * cols;
        int64_t s = 0;
        for (size_t k = 0; k < (size_t)cols * cols; ++k) s += m[k];
        m[oo] = (int64_t)counted - s;
    }
    return FNN_OK;
}

}  // extern "C"
