// label_set.h - what every kernel file that reads a label map through a label-set table shares (cc_label.h and its users,
// fill_holes_box_kernel.h, morph.hip): the block size, the table lookup and the wave sum.  No kernel lives here.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int CC_THREADS = 256;

template <typename T>
__device__ __forceinline__ int group_of(const T *labels, int i, const int *table, int n_table) {
    const int v = labels[i];
    return v < n_table ? table[v] : -1;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

inline unsigned cc_vox_blocks(int n) { return (unsigned)((n + CC_THREADS - 1) / CC_THREADS); }

}  // namespace
