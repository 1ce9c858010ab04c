// instance.hip - the connected components of a reference and a predicted label map and their overlaps, for the lesion-wise
// metrics (detection F1, false-positive / false-negative lesion volume, panoptic quality), gfx950.
//
//   fnn_instance_overlaps   per label set: the components of the reference, of the prediction, and the pieces they share
//
// Three labellings with cc_label.h's union-find (26-connectivity; its header comment holds the invariants and the memory
// rules of parent[]): the reference, the prediction, and the joint map J[v] = g + 1 where both maps' values belong to set
// g, else 0.  Two 26-adjacent voxels of J with one set lie in one component of the prediction and in one of the reference,
// so every component of J - a piece - belongs to exactly one (prediction component, reference component) pair, and the
// overlap of a pair is the sum of its pieces: the pair table needs no hash table, its memory depends only on the voxel
// count, and its order is fixed.  J is not stored: INJoint forms it from the two maps and the table on every read.  The
// labelling reads a voxel's set once in tile_merge and, for the voxels on tile faces, a few more times in cross_merge;
// both maps' values and the table's entries are in cache then, whereas a 2-byte temporary would cost one more pass that
// writes it and 2 B per voxel of scratch.
//
// After the labellings every root (parent[i] == i: the first voxel of its component in raster order) becomes one record,
// ascending in i, without an atomic cursor - the same input gives the same bytes:
//   root_count   roots per block of 1024 raster-consecutive voxels (ballots);
//   scan         exclusive scan of the blocks' counts in place, one workgroup per labelling; the totals go to the host,
//                which compares them with cap;
//   count        cc_label.h's size count, into one size array that the three labellings use in turn;
//   emit         every root's record at its block's offset plus its rank in the block (ballots).
#include "cc_label.h"
#include <climits>

namespace {

constexpr int IN_BLOCK = 1024;             // raster-consecutive voxels per block of the compaction
constexpr int IN_MAX_GROUPS = 1024;

// the loader of the joint map: the set both maps' values share, or -1
template <typename T>
struct INJoint {
    const T *ref, *pred;
    const int *table;
    __device__ __forceinline__ int group(int i, int n_table) const {
        const int a = group_of(ref, i, table, n_table);
        if (a < 0) return -1;
        return group_of(pred, i, table, n_table) == a ? a : -1;
    }
};

// ---- roots per block
__global__ __launch_bounds__(IN_BLOCK) void in_root_count_kernel(const int *parent, int n, unsigned int *counts) {
    __shared__ unsigned int wave_n[IN_BLOCK / 64];
    const long long i = (long long)blockIdx.x * IN_BLOCK + threadIdx.x;
    const bool root = i < n && parent[i] == (int)i;
    const unsigned long long vote = __ballot(root);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (unsigned int)__popcll(vote);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int t = 0;
        for (int k = 0; k < IN_BLOCK / 64; ++k) t += wave_n[k];
        counts[blockIdx.x] = t;
    }
}

// ---- exclusive scan of counts[blockIdx.x][n_blocks] in place, the sum to totals[blockIdx.x]; one workgroup per array
__global__ __launch_bounds__(IN_BLOCK) void in_scan_kernel(unsigned int *all_counts, int n_blocks, unsigned int *totals) {
    __shared__ unsigned int wave_sum[IN_BLOCK / 64];
    __shared__ unsigned int carry;
    unsigned int *counts = all_counts + (size_t)blockIdx.x * n_blocks;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n_blocks; base += IN_BLOCK) {
        const int i = base + threadIdx.x;
        const unsigned int own = i < n_blocks ? counts[i] : 0u;
        unsigned int v = own;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned int u = __shfl_up(v, o);
            if (lane >= o) v += u;
        }
        if (lane == 63) wave_sum[wave] = v;
        __syncthreads();
        unsigned int before = carry;
        for (int k = 0; k < wave; ++k) before += wave_sum[k];
        if (i < n_blocks) counts[i] = before + v - own;
        __syncthreads();
        if (threadIdx.x == IN_BLOCK - 1) carry = before + v;
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// the record index of this thread's root: the block's offset plus the roots before it in the block.  Every thread of the
// block calls it (it holds a barrier); the value means something only where root is set
__device__ __forceinline__ long long in_slot(bool root, const unsigned int *offsets, unsigned int *wave_n) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long vote = __ballot(root);
    if (lane == 0) wave_n[wave] = (unsigned int)__popcll(vote);
    __syncthreads();
    long long at = (long long)offsets[blockIdx.x] + __popcll(vote & ((1ull << lane) - 1ull));
    for (int k = 0; k < wave; ++k) at += wave_n[k];
    return at;
}

// ---- the components of one map: (set, root, size)
template <typename T>
__global__ __launch_bounds__(IN_BLOCK) void in_emit_components_kernel(CCLabelMap<T> src, int n_table, const int *parent, const int *size,
                                                                       int n, const unsigned int *offsets, int *rec, long long n_rec) {
    __shared__ unsigned int wave_n[IN_BLOCK / 64];
    const long long i = (long long)blockIdx.x * IN_BLOCK + threadIdx.x;
    const bool root = i < n && parent[i] == (int)i;
    const long long at = in_slot(root, offsets, wave_n);
    if (!root || at >= n_rec) return;
    rec[at * 3] = src.group((int)i, n_table);
    rec[at * 3 + 1] = (int)i;
    rec[at * 3 + 2] = size[i];
}

// ---- the pieces: (root of the piece's component in the prediction, in the reference, size)
__global__ __launch_bounds__(IN_BLOCK) void in_emit_pieces_kernel(const int *parent, const int *parent_pred, const int *parent_ref,
                                                                   const int *size, int n, const unsigned int *offsets, int *rec,
                                                                   long long n_rec) {
    __shared__ unsigned int wave_n[IN_BLOCK / 64];
    const long long i = (long long)blockIdx.x * IN_BLOCK + threadIdx.x;
    const bool root = i < n && parent[i] == (int)i;
    const long long at = in_slot(root, offsets, wave_n);
    if (!root || at >= n_rec) return;
    rec[at * 3] = parent_pred[i];
    rec[at * 3 + 1] = parent_ref[i];
    rec[at * 3 + 2] = size[i];
}

}  // namespace

extern "C" {

int fnn_instance_overlaps(const void *ref, const void *pred, int label_dtype, const int64_t shape[3], const int32_t *group_of_label,
                          int n_table, int n_groups, int32_t *records, int64_t cap, int64_t n_out[3], void *stream) {
    const char *who = "fnn_instance_overlaps";
    if (!shape || !n_out || (n_table > 0 && !group_of_label)) return fnn_failf(FNN_E_INVALID, "%s: NULL argument", who);
    if (int rc = fnn_check_label_dtype(label_dtype)) return rc;
    if (n_groups < 1 || n_groups > IN_MAX_GROUPS) return fnn_failf(FNN_E_INVALID, "%s: n_groups must be 1..%d", who, IN_MAX_GROUPS);
    if (n_table < 0) return fnn_failf(FNN_E_INVALID, "%s: negative n_table", who);
    for (int v = 0; v < n_table; ++v)
        if (group_of_label[v] < -1 || group_of_label[v] >= n_groups)
            return fnn_failf(FNN_E_INVALID, "%s: group_of_label entry outside [-1, n_groups)", who);
    if (shape[0] < 0 || shape[1] < 0 || shape[2] < 0) return fnn_failf(FNN_E_INVALID, "%s: negative extent", who);
    if (cap < 0) return fnn_failf(FNN_E_INVALID, "%s: cap is negative", who);
    n_out[0] = n_out[1] = n_out[2] = 0;
    if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return FNN_OK;
    if (shape[0] > INT_MAX || shape[1] > INT_MAX || shape[2] > INT_MAX || shape[0] * shape[1] > INT_MAX ||
        shape[0] * shape[1] * shape[2] > INT_MAX)
        return fnn_failf(FNN_E_UNSUPPORTED, "%s: more than 2^31 - 1 voxels", who);
    const uintptr_t emask = label_dtype == FNN_LABEL_U16 ? 1 : 0;
    if (ref && pred && (((uintptr_t)ref | (uintptr_t)pred) & emask)) return fnn_failf(FNN_E_INVALID, "%s: label maps must be aligned to their element", who);
    if (records && ((uintptr_t)records & 3)) return fnn_failf(FNN_E_INVALID, "%s: records must be 4-byte aligned", who);
    if (int rc = fnn_need_dev(who, {ref, pred, records}, "device pointers for ref, pred and records")) return rc;
    const int max_label = label_dtype == FNN_LABEL_U16 ? 65535 : 255;
    const int n_tab = n_table < max_label + 1 ? n_table : max_label + 1;      // labels the dtype cannot hold are never looked up
    if (n_tab == 0) return FNN_OK;                                               // no value in any set: no component
    const int n = (int)(shape[0] * shape[1] * shape[2]);
    const CCGeom g = cc_geom(shape, n_tab);
    const int n_blocks = (int)(((long long)n + IN_BLOCK - 1) / IN_BLOCK);

    // one scratch block: parent of ref, pred, joint [3][n] | size [n] | counts [3][n_blocks] | totals [3] | table [n_tab]
    const size_t off_size = (size_t)n * 12, off_counts = off_size + (size_t)n * 4, off_totals = off_counts + (size_t)n_blocks * 12;
    const size_t off_table = off_totals + 12;
    DevBuf scratch;
    if (!scratch.alloc(off_table + (size_t)n_tab * 4)) return fnn_failf(FNN_E_HIP, "hipMalloc failed (%s: 16 B per voxel of scratch)", who);
    int *parent[3] = {scratch.as<int>(), scratch.as<int>((size_t)n * 4), scratch.as<int>((size_t)n * 8)};
    int *size = scratch.as<int>(off_size), *table = scratch.as<int>(off_table);
    unsigned int *counts = scratch.as<unsigned int>(off_counts), *totals = scratch.as<unsigned int>(off_totals);
    HipCall call(stream);
    call.copy(table, group_of_label, (size_t)n_tab * 4, hipMemcpyHostToDevice);
    fnn_by_label(label_dtype, [&](auto lt) {
        using T = decltype(lt);
        cc_label(call, CCLabelMap<T>{(const T *)ref, table}, g, n, parent[0]);
        cc_label(call, CCLabelMap<T>{(const T *)pred, table}, g, n, parent[1]);
        cc_label(call, INJoint<T>{(const T *)ref, (const T *)pred, table}, g, n, parent[2]);
    });
    for (int k = 0; k < 3; ++k)
        call.launch(in_root_count_kernel, dim3((unsigned)n_blocks), dim3(IN_BLOCK), 0, (const int *)parent[k], n, counts + (size_t)k * n_blocks);
    call.launch(in_scan_kernel, dim3(3), dim3(IN_BLOCK), 0, counts, n_blocks, totals);
    unsigned int htot[3] = {0, 0, 0};
    call.copy(htot, totals, sizeof htot, hipMemcpyDeviceToHost);
    if (!call.sync()) return call.fail();
    for (int k = 0; k < 3; ++k) n_out[k] = (int64_t)htot[k];
    const long long total = (long long)htot[0] + htot[1] + htot[2];
    if (cap < total || total == 0) return FNN_OK;                                // too small: nothing is written

    fnn_by_label(label_dtype, [&](auto lt) {
        using T = decltype(lt);
        long long at = 0;
        for (int k = 0; k < 3; ++k) {
            const unsigned int *offsets = counts + (size_t)k * n_blocks;
            int *rec = records + at * 3;
            call.fill(size, 0, (size_t)n * 4);
            cc_sizes(call, parent[k], n, size);
            if (k < 2)
                call.launch(in_emit_components_kernel<T>, dim3((unsigned)n_blocks), dim3(IN_BLOCK), 0,
                            CCLabelMap<T>{(const T *)(k ? pred : ref), table}, n_tab, (const int *)parent[k], (const int *)size, n, offsets,
                            rec, (long long)htot[k]);
            else
                call.launch(in_emit_pieces_kernel, dim3((unsigned)n_blocks), dim3(IN_BLOCK), 0, (const int *)parent[2], (const int *)parent[1],
                            (const int *)parent[0], (const int *)size, n, offsets, rec, (long long)htot[k]);
            at += htot[k];
        }
    });
    return call.finish();
}

}  // extern "C"
