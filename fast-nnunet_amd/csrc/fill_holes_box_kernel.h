// fill_holes_box_kernel.h - the box pass that fnn_fill_holes (postprocess.hip) and fnn_binary_morphology (morph.hip) share:
// one launch that leaves the bounding box of a label set S and its voxel count in the form fill_holes_box.h reads
// (fh_box_from_raw).  Device code; the arithmetic on the result is fill_holes_box.h's, host code without HIP.
#pragma once
#include "host_call.h"
#include "label_set.h"
#include "fill_holes_box.h"

namespace {

struct FHVolume { int X, Y, Z; };

template <typename T>
__device__ __forceinline__ bool fh_in_set(const T *labels, int i, const int *table, int n_table) {
    return group_of(labels, i, table, n_table) >= 0;
}

// the box of S: raw[k] = (extent of axis k) - 1 - lowest coordinate, raw[3 + k] = highest coordinate (both grow, so the
// buffer starts as all -1), and the number of voxels of S
template <typename T>
__global__ __launch_bounds__(CC_THREADS) void fh_box_kernel(const T *labels, const int *table, int n_table, FHVolume v, int *raw,
                                                            unsigned long long *count) {
    __shared__ int sraw[6];
    __shared__ unsigned int scount;
    if (threadIdx.x < 6) sraw[threadIdx.x] = -1;
    if (threadIdx.x == 6) scount = 0;
    __syncthreads();
    const long long n = (long long)v.X * v.Y * v.Z;
    int mine[6] = {-1, -1, -1, -1, -1, -1};
    unsigned int cnt = 0;
    for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CC_THREADS) {
        if (!fh_in_set(labels, (int)i, table, n_table)) continue;
        const int z = (int)(i % v.Z), t = (int)(i / v.Z), y = t % v.Y, x = t / v.Y;
        mine[0] = max(mine[0], v.X - 1 - x); mine[1] = max(mine[1], v.Y - 1 - y); mine[2] = max(mine[2], v.Z - 1 - z);
        mine[3] = max(mine[3], x); mine[4] = max(mine[4], y); mine[5] = max(mine[5], z);
        ++cnt;
    }
    if (cnt) {
#pragma unroll
        for (int k = 0; k < 6; ++k) atomicMax(sraw + k, mine[k]);
        atomicAdd(&scount, cnt);
    }
    __syncthreads();
    if (threadIdx.x < 6 && sraw[threadIdx.x] >= 0) atomicMax(raw + threadIdx.x, sraw[threadIdx.x]);
    if (threadIdx.x == 6 && scount) atomicAdd(count, (unsigned long long)scount);
}

// the launch of the box pass on the call's stream: raw [8 ints, 6 used] and count [1] start as all -1 and 0
template <typename T>
inline void fh_launch_box(HipCall &call, const T *labels, const int *table, int n_table, const FHVolume &v, int *raw,
                          unsigned long long *count) {
    const unsigned vox_blocks = cc_vox_blocks(v.X * v.Y * v.Z);
    call.launch(fh_box_kernel<T>, dim3(vox_blocks < 2048u ? vox_blocks : 2048u), dim3(CC_THREADS), 0, labels, table, n_table, v, raw,
                count);
}

}  // namespace
