// postprocess.hip - nnU-Net's connected-component postprocessing on the label map, gfx950.
//
//   fnn_keep_largest_components   remove_all_but_largest_component_from_segmentation
//                                 (postprocessing/remove_connected_components.py:21-33) for several disjoint label
//                                 sets in one pass
//
// Label-aware 3-D connected components (26-connectivity) by union-find over int32 voxel indices, in six launches; the
// first four are cc_label.h's (its header comment holds the invariants and the memory rules of parent[]):
//   1. tile_merge    init + union inside a 1024-voxel tile through LDS;
//   2. cross_merge   the backward neighbours outside the voxel's tile, linked lock-free;
//   3. flatten       parent[i] = root(i);
//   4. count         size[root] += 1, aggregated per thread run and per wave before the atomic;
//   5. group_max     per set, the largest component size (atomicMax by roots, through an LDS table per workgroup);
//   6. apply         voxels of a set whose component is smaller than the set's maximum become background_label.
#include "cc_label.h"
#include <climits>
#include <vector>

namespace {

constexpr int CC_LDS_GROUPS = 4096;    // sets counted through an LDS table per workgroup (more: straight global atomics)

// 5. per set, the largest component
template <typename T>
__global__ __launch_bounds__(CC_THREADS) void cc_group_max_kernel(const T *labels, const int *table, int n_table, const int *parent,
                                                                  const int *size, int n, int n_groups, int *gmax) {
    __shared__ int smax[CC_LDS_GROUPS];
    const bool lds = n_groups <= CC_LDS_GROUPS;
    if (lds) {
        for (int k = threadIdx.x; k < n_groups; k += CC_THREADS) smax[k] = 0;
        __syncthreads();
    }
    for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CC_THREADS) {
        if (parent[i] != i) continue;
        const int grp = group_of(labels, (int)i, table, n_table);
        if (lds) atomicMax(smax + grp, size[i]);
        else atomicMax(gmax + grp, size[i]);
    }
    if (lds) {
        __syncthreads();
        for (int k = threadIdx.x; k < n_groups; k += CC_THREADS)
            if (smax[k] > 0) atomicMax(gmax + k, smax[k]);
    }
}

// 6. everything of a set outside its largest components becomes background; removed voxels counted per set
template <typename T>
__global__ __launch_bounds__(CC_THREADS) void cc_apply_kernel(T *labels, const int *table, int n_table, const int *parent,
                                                              const int *size, const int *gmax, int n, int n_groups, T background,
                                                              unsigned long long *removed) {
    __shared__ int srem[CC_LDS_GROUPS];
    const bool lds = n_groups <= CC_LDS_GROUPS;
    if (lds) {
        for (int k = threadIdx.x; k < n_groups; k += CC_THREADS) srem[k] = 0;
        __syncthreads();
    }
    for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CC_THREADS) {
        const int r = parent[i];
        if (r < 0) continue;
        const int grp = group_of(labels, (int)i, table, n_table);
        if (size[r] == gmax[grp]) continue;
        labels[i] = background;
        if (lds) atomicAdd(srem + grp, 1);
        else atomicAdd(removed + grp, 1ull);
    }
    if (lds) {
        __syncthreads();
        for (int k = threadIdx.x; k < n_groups; k += CC_THREADS)
            if (srem[k] > 0) atomicAdd(removed + k, (unsigned long long)srem[k]);
    }
}

template <typename T>
void launch_all(T *labels, const int *table, const CCGeom &g, int n, int n_groups, T background, int *parent, int *size,
                int *gmax, unsigned long long *removed, HipCall &call) {
    const unsigned vox_blocks = cc_vox_blocks(n);
    const unsigned red_blocks = vox_blocks < 2048u ? vox_blocks : 2048u;
    const dim3 block(CC_THREADS);
    cc_label(call, CCLabelMap<T>{labels, table}, g, n, parent);
    cc_sizes(call, parent, n, size);
    call.launch(cc_group_max_kernel<T>, dim3(red_blocks), block, 0, labels, table, g.n_table, parent,
                size, n, n_groups, gmax);
    call.launch(cc_apply_kernel<T>, dim3(red_blocks), block, 0, labels, table, g.n_table, parent, size,
                gmax, n, n_groups, background, removed);
}

}  // namespace

extern "C" {

int fnn_keep_largest_components(void *labels, int label_dtype, const int64_t shape[3], const int32_t *group_of_label, int n_table,
                                int n_groups, int background_label, int64_t *removed, void *stream) {
    if (!shape) return fnn_fail(FNN_E_INVALID, "NULL shape");
    if (int rc = fnn_check_label_dtype(label_dtype)) return rc;
    const int max_label = label_dtype == FNN_LABEL_U16 ? 65535 : 255;
    if (background_label < 0 || background_label > max_label) return fnn_fail(FNN_E_INVALID, "background_label outside the label dtype");
    if (shape[0] < 0 || shape[1] < 0 || shape[2] < 0) return fnn_fail(FNN_E_INVALID, "negative shape");
    if (n_groups < 0 || n_table < 0 || (n_table > 0 && !group_of_label)) return fnn_fail(FNN_E_INVALID, "bad label-set table");
    for (int v = 0; v < n_table; ++v)
        if (group_of_label[v] < -1 || group_of_label[v] >= n_groups) return fnn_fail(FNN_E_INVALID, "group_of_label entry outside [-1, n_groups)");
    if (removed)
        for (int k = 0; k < n_groups; ++k) removed[k] = 0;
    if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return FNN_OK;
    if (shape[0] > INT_MAX || shape[1] > INT_MAX || shape[2] > INT_MAX || shape[0] * shape[1] > INT_MAX ||
        shape[0] * shape[1] * shape[2] > INT_MAX)
        return fnn_fail(FNN_E_UNSUPPORTED, "fnn_keep_largest_components: more than 2^31 - 1 voxels");
    if (int rc = fnn_need_dev("fnn_keep_largest_components", {labels}, "a device label map")) return rc;
    const int n_tab = n_table < max_label + 1 ? n_table : max_label + 1;      // labels the dtype cannot hold are never looked up
    if (n_groups == 0 || n_tab == 0) return FNN_OK;                              // no set: nothing changes
    const int n = (int)(shape[0] * shape[1] * shape[2]);

    const CCGeom g = cc_geom(shape, n_tab);

    // one scratch block: parent [n] | size [n] | table [n_tab] | gmax [n_groups] | removed [n_groups] (8-B aligned)
    const size_t off_size = (size_t)n * 4, off_table = off_size + (size_t)n * 4, off_gmax = off_table + (size_t)n_tab * 4;
    const size_t off_removed = (off_gmax + (size_t)n_groups * 4 + 7) & ~(size_t)7;
    DevBuf scratch;
    if (!scratch.alloc(off_removed + (size_t)n_groups * 8)) return fnn_fail(FNN_E_HIP, "hipMalloc failed (8 B per voxel of scratch)");
    int *parent = scratch.as<int>(), *size = scratch.as<int>(off_size), *table = scratch.as<int>(off_table), *gmax = scratch.as<int>(off_gmax);
    unsigned long long *rem = scratch.as<unsigned long long>(off_removed);
    HipCall call(stream);
    call.copy(table, group_of_label, (size_t)n_tab * 4, hipMemcpyHostToDevice);
    call.fill(size, 0, (size_t)n * 4);
    call.fill(gmax, 0, (size_t)(off_removed - off_gmax) + (size_t)n_groups * 8);
    fnn_by_label(label_dtype, [&](auto lt) {
        using LT = decltype(lt);
        launch_all<LT>((LT *)labels, table, g, n, n_groups, (LT)background_label, parent, size, gmax, rem, call);
    });
    std::vector<unsigned long long> hrem(removed ? (size_t)n_groups : 0);
    if (removed) call.copy(hrem.data(), rem, (size_t)n_groups * 8, hipMemcpyDeviceToHost);
    if (!call.sync()) return call.fail();
    for (size_t k = 0; k < hrem.size(); ++k) removed[k] = (int64_t)hrem[k];
    return FNN_OK;
}

}  // extern "C"
