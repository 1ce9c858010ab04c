// postprocess.hip - nnU-Net's connected-component postprocessing on the label map, gfx950.
//
//   fnn_keep_largest_components   remove_all_but_largest_component_from_segmentation
//                                 (postprocessing/remove_connected_components.py:21-33) for several disjoint label
//                                 sets in one pass
//   fnn_remove_small_components   per set, every component below the set's min_size becomes background (26- or
//                                 6-connectivity); the rule is scipy's ndimage.label + bincount
//   fnn_fill_holes                scipy's binary_fill_holes of one label set: background voxels in its holes get fill_label
//
// Label-aware 3-D connected components (26-connectivity) by union-find over int32 voxel indices, in six launches; the
// first four are cc_label.h's (its header comment holds the invariants and the memory rules of parent[]):
//   1. tile_merge    init + union inside a 1024-voxel tile through LDS;
//   2. cross_merge   the backward neighbours outside the voxel's tile, linked lock-free;
//   3. flatten       parent[i] = root(i);
//   4. count         size[root] += 1, aggregated per thread run and per wave before the atomic;
//   5. group_max     per set, the largest component size (atomicMax by roots, through an LDS table per workgroup);
//   6. apply         voxels of a set whose component is smaller than the set's maximum become background_label.
// fnn_remove_small_components is 1-4 and 6 with the sets' min_size in the place of the maxima (no launch 5).
//
// fnn_fill_holes, five launches and one host read in between:
//   a. box           the bounding box of the set S and its voxel count (LDS atomics per workgroup, then six global ones;
//                    fill_holes_box_kernel.h, shared with morph.hip);
//                    the host reads it: an empty S, or S filling its box, ends the call;
//   1-3.             cc_label.h with 6-connectivity on the complement of S inside the box (a loader that maps box-local
//                    indices to voxels); fill_holes_box.h says why the box is enough and which of its faces open a component;
//   b. mark          open[root] = 1 for every complement voxel on an opening box face (the same plain store from many threads);
//   c. fill          voxels of components that were not marked and whose value is background_label become fill_label.
#include "cc_label.h"
#include "fill_holes_box_kernel.h"
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

// 6. everything of a set outside the components it keeps becomes background; removed voxels counted per set.  A component is
// kept if its size equals keep[set] (the set's maximum), or with MIN_SIZE if it is at least keep[set] (the set's min_size,
// an unsigned value up to 2^31)
template <typename T, bool MIN_SIZE>
__global__ __launch_bounds__(CC_THREADS) void cc_apply_kernel(T *labels, const int *table, int n_table, const int *parent,
                                                              const int *size, const int *keep, int n, int n_groups, T background,
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
        if (MIN_SIZE ? (unsigned)size[r] >= (unsigned)keep[grp] : size[r] == keep[grp]) continue;
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

// keep the largest (MIN_SIZE false: gmax is zero and launch 5 fills it) or everything of at least min_size (gmax holds it)
template <typename T, int CONN, bool MIN_SIZE>
void launch_all(T *labels, const int *table, const CCGeom &g, int n, int n_groups, T background, int *parent, int *size,
                int *gmax, unsigned long long *removed, HipCall &call) {
    const unsigned vox_blocks = cc_vox_blocks(n);
    const unsigned red_blocks = vox_blocks < 2048u ? vox_blocks : 2048u;
    const dim3 block(CC_THREADS);
    cc_label<CCLabelMap<T>, CONN>(call, CCLabelMap<T>{labels, table}, g, n, parent);
    cc_sizes(call, parent, n, size);
    if (!MIN_SIZE)
        call.launch(cc_group_max_kernel<T>, dim3(red_blocks), block, 0, labels, table, g.n_table, parent,
                    size, n, n_groups, gmax);
    call.launch(cc_apply_kernel<T, MIN_SIZE>, dim3(red_blocks), block, 0, labels, table, g.n_table, parent, size,
                gmax, n, n_groups, background, removed);
}

// what fnn_keep_largest_components (min_size NULL, 26-connectivity) and fnn_remove_small_components share: the refusals,
// the scratch and the launches
int components_call(const char *who, void *labels, int label_dtype, const int64_t shape[3], const int32_t *group_of_label,
                    int n_table, int n_groups, int background_label, const int64_t *min_size, int connectivity,
                    int64_t *removed, void *stream) {
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
        return fnn_failf(FNN_E_UNSUPPORTED, "%s: more than 2^31 - 1 voxels", who);
    if (int rc = fnn_need_dev(who, {labels}, "a device label map")) return rc;
    const int n_tab = n_table < max_label + 1 ? n_table : max_label + 1;      // labels the dtype cannot hold are never looked up
    if (n_groups == 0 || n_tab == 0) return FNN_OK;                              // no set: nothing changes
    const int n = (int)(shape[0] * shape[1] * shape[2]);

    // min_size as the unsigned value the kernel compares with: no component is larger than 2^31 - 1 voxels
    std::vector<unsigned int> keep;
    if (min_size) {
        bool any = false;
        for (int k = 0; k < n_groups; ++k) {
            keep.push_back(min_size[k] < 0 ? 0u : min_size[k] > (int64_t)INT_MAX ? 0x80000000u : (unsigned int)min_size[k]);
            any |= min_size[k] > 1;
        }
        if (!any) return FNN_OK;                                                 // every min_size <= 1: nothing changes
    }

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
    if (min_size) call.copy(gmax, keep.data(), (size_t)n_groups * 4, hipMemcpyHostToDevice);
    fnn_by_label(label_dtype, [&](auto lt) {
        using LT = decltype(lt);
        LT *const map = (LT *)labels;
        const LT bg = (LT)background_label;
        if (!min_size) launch_all<LT, 26, false>(map, table, g, n, n_groups, bg, parent, size, gmax, rem, call);
        else if (connectivity == 6) launch_all<LT, 6, true>(map, table, g, n, n_groups, bg, parent, size, gmax, rem, call);
        else launch_all<LT, 26, true>(map, table, g, n, n_groups, bg, parent, size, gmax, rem, call);
    });
    std::vector<unsigned long long> hrem(removed ? (size_t)n_groups : 0);
    if (removed) call.copy(hrem.data(), rem, (size_t)n_groups * 8, hipMemcpyDeviceToHost);
    if (!call.sync()) return call.fail();
    for (size_t k = 0; k < hrem.size(); ++k) removed[k] = (int64_t)hrem[k];
    return FNN_OK;
}

// ---- fnn_fill_holes
// the loader of the complement of S inside the box: voxel i of the box in raster order is in set 0 unless its value is in S
template <typename T>
struct CCBoxComplement {
    const T *labels;
    const int *table;
    FHBox b;
    int Y, Z;
    __device__ __forceinline__ int voxel(int i) const {
        const int z = i % b.bz, t = i / b.bz, y = t % b.by, x = t / b.by;
        return ((b.x0 + x) * Y + (b.y0 + y)) * Z + (b.z0 + z);
    }
    __device__ __forceinline__ int group(int i, int n_table) const { return fh_in_set(labels, voxel(i), table, n_table) ? -1 : 0; }
};

// b. a complement component with a voxel on an opening face of the box is no hole
__global__ __launch_bounds__(CC_THREADS) void fh_mark_kernel(const int *parent, FHBox b, int open_faces, int n_box, int *open) {
    for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < n_box; i += (long long)gridDim.x * CC_THREADS) {
        const int l = (int)i, z = l % b.bz, t = l / b.bz, y = t % b.by, x = t / b.by;
        const int on = (x == 0 ? 1 : 0) | (x == b.bx - 1 ? 2 : 0) | (y == 0 ? 4 : 0) | (y == b.by - 1 ? 8 : 0) | (z == 0 ? 16 : 0) |
                       (z == b.bz - 1 ? 32 : 0);
        if (!(on & open_faces)) continue;
        const int r = parent[l];
        if (r >= 0) open[r] = 1;
    }
}

// c. background voxels of the holes become fill
template <typename T>
__global__ __launch_bounds__(CC_THREADS) void fh_fill_kernel(T *labels, CCBoxComplement<T> src, const int *parent, const int *open,
                                                             int n_box, T background, T fill, unsigned long long *filled) {
    int cnt = 0;
    for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < n_box; i += (long long)gridDim.x * CC_THREADS) {
        const int r = parent[i];
        if (r < 0 || open[r]) continue;
        const int vox = src.voxel((int)i);
        if (labels[vox] != background) continue;
        labels[vox] = fill;
        ++cnt;
    }
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(filled, (unsigned long long)cnt);
}

}  // namespace

extern "C" {

int fnn_keep_largest_components(void *labels, int label_dtype, const int64_t shape[3], const int32_t *group_of_label, int n_table,
                                int n_groups, int background_label, int64_t *removed, void *stream) {
    return components_call("fnn_keep_largest_components", labels, label_dtype, shape, group_of_label, n_table, n_groups,
                           background_label, nullptr, 26, removed, stream);
}

int fnn_remove_small_components(void *labels, int label_dtype, const int64_t shape[3], const int32_t *group_of_label, int n_table,
                                int n_groups, int background_label, const int64_t *min_size, int connectivity, int64_t *removed,
                                void *stream) {
    if (connectivity != 6 && connectivity != 26) return fnn_fail(FNN_E_UNSUPPORTED, "fnn_remove_small_components: connectivity must be 6 or 26");
    if (!min_size) return fnn_fail(FNN_E_INVALID, "NULL min_size");
    return components_call("fnn_remove_small_components", labels, label_dtype, shape, group_of_label, n_table, n_groups,
                           background_label, min_size, connectivity, removed, stream);
}

int fnn_fill_holes(void *labels, int label_dtype, const int64_t shape[3], const int32_t *group_of_label, int n_table,
                   int background_label, int fill_label, int border_axes, int64_t *filled, void *stream) {
    const char *who = "fnn_fill_holes";
    if (!shape) return fnn_fail(FNN_E_INVALID, "NULL shape");
    if (int rc = fnn_check_label_dtype(label_dtype)) return rc;
    const int max_label = label_dtype == FNN_LABEL_U16 ? 65535 : 255;
    if (background_label < 0 || background_label > max_label) return fnn_fail(FNN_E_INVALID, "background_label outside the label dtype");
    if (fill_label < 0 || fill_label > max_label) return fnn_fail(FNN_E_INVALID, "fill_label outside the label dtype");
    if (fill_label == background_label) return fnn_fail(FNN_E_INVALID, "fill_label equals background_label");
    if (border_axes < 1 || border_axes > 7) return fnn_fail(FNN_E_INVALID, "border_axes must be 1..7 (bit a: axis a has borders)");
    if (shape[0] < 0 || shape[1] < 0 || shape[2] < 0) return fnn_fail(FNN_E_INVALID, "negative shape");
    if (n_table < 0 || (n_table > 0 && !group_of_label)) return fnn_fail(FNN_E_INVALID, "bad label-set table");
    for (int v = 0; v < n_table; ++v)
        if (group_of_label[v] < -1 || group_of_label[v] > 0) return fnn_fail(FNN_E_INVALID, "group_of_label entry outside [-1, 0]");
    if (filled) *filled = 0;
    if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return FNN_OK;
    if (shape[0] > INT_MAX || shape[1] > INT_MAX || shape[2] > INT_MAX || shape[0] * shape[1] > INT_MAX ||
        shape[0] * shape[1] * shape[2] > INT_MAX)
        return fnn_failf(FNN_E_UNSUPPORTED, "%s: more than 2^31 - 1 voxels", who);
    if (int rc = fnn_need_dev(who, {labels}, "a device label map")) return rc;
    const int n_tab = n_table < max_label + 1 ? n_table : max_label + 1;
    if (n_tab == 0) return FNN_OK;                                               // S is empty
    const FHVolume vol{(int)shape[0], (int)shape[1], (int)shape[2]};

    // the small block: raw box [6] | pad [2] | voxels of S | filled | table [n_tab]
    DevBuf small;
    if (!small.alloc(48 + (size_t)n_tab * 4)) return fnn_fail(FNN_E_HIP, "hipMalloc failed (fnn_fill_holes: the label table)");
    int *raw = small.as<int>(), *table = small.as<int>(48);
    unsigned long long *count = small.as<unsigned long long>(32), *nfilled = small.as<unsigned long long>(40);
    HipCall call(stream);
    call.fill(raw, 0xff, 32);
    call.fill(count, 0, 16);
    call.copy(table, group_of_label, (size_t)n_tab * 4, hipMemcpyHostToDevice);
    const dim3 block(CC_THREADS);
    fnn_by_label(label_dtype, [&](auto lt) {
        using LT = decltype(lt);
        fh_launch_box(call, (const LT *)labels, table, n_tab, vol, raw, count);
    });
    struct { int raw[8]; unsigned long long count; } found;
    call.copy(&found, raw, 40, hipMemcpyDeviceToHost);
    if (!call.sync()) return call.fail();
    FHBox b;
    if (!fh_box_from_raw(found.raw, shape, b)) return FNN_OK;                     // S is empty
    if ((int64_t)found.count == fh_box_voxels(b)) return FNN_OK;                  // S fills its box: no complement inside it
    const int n_box = (int)fh_box_voxels(b);
    const int open_faces = fh_open_faces(b, shape, border_axes);

    // parent [n_box] | open [n_box]
    DevBuf scratch;
    if (!scratch.alloc((size_t)n_box * 8)) return fnn_fail(FNN_E_HIP, "hipMalloc failed (fnn_fill_holes: 8 B per voxel of the set's box)");
    int *parent = scratch.as<int>(), *open = scratch.as<int>((size_t)n_box * 4);
    call.fill(open, 0, (size_t)n_box * 4);
    const int64_t box_shape[3] = {b.bx, b.by, b.bz};
    const CCGeom g = cc_geom(box_shape, n_tab);
    const unsigned box_blocks = cc_vox_blocks(n_box), red_blocks = box_blocks < 2048u ? box_blocks : 2048u;
    fnn_by_label(label_dtype, [&](auto lt) {
        using LT = decltype(lt);
        const CCBoxComplement<LT> src{(const LT *)labels, table, b, vol.Y, vol.Z};
        cc_label<CCBoxComplement<LT>, 6>(call, src, g, n_box, parent);
        call.launch(fh_mark_kernel, dim3(red_blocks), block, 0, (const int *)parent, b, open_faces, n_box, open);
        call.launch(fh_fill_kernel<LT>, dim3(red_blocks), block, 0, (LT *)labels, src, (const int *)parent, (const int *)open, n_box,
                    (LT)background_label, (LT)fill_label, nfilled);
    });
    unsigned long long hfilled = 0;
    if (filled) call.copy(&hfilled, nfilled, 8, hipMemcpyDeviceToHost);
    if (!call.sync()) return call.fail();
    if (filled) *filled = (int64_t)hfilled;
    return FNN_OK;
}

}  // extern "C"

