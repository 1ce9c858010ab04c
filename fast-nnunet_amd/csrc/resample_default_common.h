// resample_default_common.h - the arithmetic of the default resampling family at order 1 / order_z 0 (interp_kernel of
// resample.hip, fp64), once: what export_labels.hip (labels straight from the logits of the network grid) and
// ensemble_resample.hip (the ensemble's average straight from the members' network grids) must agree on bit for bit.
// The expressions and why each has its form are described at the top of export_labels.hip.
#pragma once
#include "fnn_device.h"
#include <cmath>

struct DGeo {
    long long in[3], out[3];
    double zoom[3];            // (double)in / (double)out
    int sep;                   // the order-0 axis or -1
    unsigned plane_blocks;     // blocks of 256 output voxels per x slab
    unsigned plane;            // out[1] * out[2]
};

// taps and weights of output index o along axis a; TWO: the axis interpolates
template <bool TWO>
static __device__ __forceinline__ void d_axis(const DGeo &g, int a, long long o, long long (&i)[2], double (&w)[2]) {
#pragma clang fp contract(off)
    const long long n = g.in[a];
    if (!TWO) {
        long long s = o;                                       // in == out
        if (n != g.out[a]) {                                   // the separate axis: map_coordinates(order 0, mode 'nearest')
            const double x = fma((double)o + 0.5, g.zoom[a], -0.5);
            s = (long long)floor(x + 0.5);
            s = s < 0 ? 0 : (s >= n ? n - 1 : s);
        }
        i[0] = i[1] = s; w[0] = 1.0; w[1] = 0.0;
        return;
    }
    double x = fma((double)o, g.zoom[a], 0.5 * g.zoom[a] - 0.5);
    x = x < 0 ? 0 : (x > (double)(n - 1) ? (double)(n - 1) : x);             // mode 'nearest'
    const double f = floor(x), t = x - f;
    i[0] = (long long)f;
    i[1] = i[0] + 1 >= n ? n - 1 : i[0] + 1;
    w[0] = 1.0 - t; w[1] = t;
}

// one head's value from its taps v (index = tap of axis 0, then 1, then 2; only the taps of M are there)
template <typename T, int M>
static __device__ __forceinline__ float d_value(const T (&v)[8], const double (&w)[3][2]) {
#pragma clang fp contract(off)
    constexpr int N0 = (M & 1) ? 2 : 1, N1 = (M & 2) ? 2 : 1, N2 = (M & 4) ? 2 : 1;
    double acc = 0;
#pragma unroll
    for (int a0 = 0; a0 < N0; ++a0)
#pragma unroll
        for (int a1 = 0; a1 < N1; ++a1)
#pragma unroll
            for (int a2 = 0; a2 < N2; ++a2) {
                double t = (double)v[a0 * 4 + a1 * 2 + a2];
                if (M & 1) t = t * w[0][a0];
                if (M & 2) t = t * w[1][a1];
                acc = (M & 4) ? fma(t, w[2][a2], acc) : acc + t;
            }
    return (float)(T)acc;                                      // rounded once to the logits' dtype, like the stored tensor
}
